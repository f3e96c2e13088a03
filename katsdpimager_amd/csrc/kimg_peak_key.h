// The peak key of the CLEAN kernels (clean.hip, clean_multi.hip, clean_scales.hip) and its
// reductions.  Everything here is local to the including translation unit.
#pragma once
#include "kimg_common.h"

namespace {

// (value, index) as one unsigned key that orders like the reference's selection: larger value
// first, then smaller index.  Values are non-negative floats (never NaN: a NaN metric never
// replaces a tile's best), whose bit patterns order like the numbers.  Key 0 = nothing.
typedef unsigned long long key_t;

__device__ inline key_t make_key(float value, int idx)
{
    return ((key_t) __float_as_uint(value) << 32) | (unsigned) ~idx;
}

__device__ inline key_t key_max(key_t a, key_t b) { return a > b ? a : b; }

template <int CTRL>
__device__ inline key_t key_dpp(key_t k)        // lanes without a source read 0
{
    const unsigned lo = __builtin_amdgcn_mov_dpp((unsigned) k, CTRL, 0xf, 0xf, true);
    const unsigned hi = __builtin_amdgcn_mov_dpp((unsigned) (k >> 32), CTRL, 0xf, 0xf, true);
    return ((key_t) hi << 32) | lo;
}

// Maximum over each 16-lane row, in every lane of the row (DPP butterflies: ALU latency only)
__device__ inline key_t row_max_key(key_t k)
{
    k = key_max(k, key_dpp<0xB1>(k));       // quad_perm [1,0,3,2]
    k = key_max(k, key_dpp<0x4E>(k));       // quad_perm [2,3,0,1]
    k = key_max(k, key_dpp<0x141>(k));      // row_half_mirror
    k = key_max(k, key_dpp<0x140>(k));      // row_mirror
    return k;
}

__device__ inline key_t read_lane_key(key_t k, int lane)
{
    return ((key_t) (unsigned) __builtin_amdgcn_readlane((int) (k >> 32), lane) << 32)
           | (unsigned) __builtin_amdgcn_readlane((int) k, lane);
}

// Maximum over a wave, the same (uniform) value in every lane.  All 64 lanes must be active.
__device__ inline key_t wave_max_key(key_t k)
{
    k = row_max_key(k);
    return key_max(key_max(read_lane_key(k, 0), read_lane_key(k, 16)),
                   key_max(read_lane_key(k, 32), read_lane_key(k, 48)));
}

// A workgroup barrier that orders LDS traffic only: __syncthreads() also waits for every global
// store of the wave (its release semantics), which puts the latency of stores nobody is waiting
// for on a latency-critical chain.
__device__ inline void lds_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// Maximum over a block of up to 1024 threads (a multiple of 64), the same (uniform) value in
// every thread.  `s_keys` [waves of the block] is shared scratch; two uses must be separated by a
// barrier.  LDS_ONLY: the barrier inside is lds_barrier() instead of __syncthreads().
template <bool LDS_ONLY = false>
__device__ inline key_t block_max_key(key_t k, key_t *s_keys)
{
    const key_t w = wave_max_key(k);
    if ((threadIdx.x & 63) == 0)
        s_keys[threadIdx.x >> 6] = w;
    if (LDS_ONLY)
        lds_barrier();
    else
        __syncthreads();
    const int nw = blockDim.x >> 6, e = threadIdx.x & 15;
    k = row_max_key(e < nw ? s_keys[e] : 0);
    return read_lane_key(k, 0);
}

// Record `t` of the tile arrays, for the 32 x 32 tile whose first pixel is (x0, y0), from the
// maximum `k` of make_key(metric, row-major index within the tile) over its pixels with a positive
// metric: value and (y, x) of the first strict maximum in row-major order (clean.py:953-958), or
// -- nothing above 0 -- value 0 and the start position, stored the way the reference stores it:
// best_pos = (x0, y0) (clean.py:950).  (Indexed by `t`, not handed two pointers: the two-launch
// loop's subtract/update kernels then compile to the code they had with the decode spelled out.)
template <class INDEX>
__device__ inline void store_tile_record(key_t k, int x0, int y0, float *tile_max, int32_t *tile_pos,
                                         INDEX t)
{
    if (k == 0) {
        tile_max[t] = 0.0f;
        tile_pos[2 * t] = x0;
        tile_pos[2 * t + 1] = y0;
    } else {
        const int idx = ~(int) (unsigned) k;
        tile_max[t] = __uint_as_float((unsigned) (k >> 32));
        tile_pos[2 * t] = y0 + (idx >> 5);
        tile_pos[2 * t + 1] = x0 + (idx & 31);
    }
}

} // namespace
