// What the column walks over a cube [C][M] of image planes share (moments.hip, imcontsub.hip): a
// thread owns V consecutive elements of the plane (V = 4 with 16-byte loads and stores, or 1) for a
// whole channel loop, so nothing crosses threads and the order of every sum is the loop's.  Here are
// the V-wide load and store, the per-channel bit mask that travels by value and its reader, and the
// host's split of a plane into the part the 16-byte form takes and the tail.  What a unit adds up, and
// in which order, is its own contract.  Everything here is local to the including translation unit.
#pragma once
#include "kimg_common.h"

namespace {

constexpr int COL_THREADS = 256;
constexpr int COL_MAX_CHANNELS = KIMG_MOMENTS_MAX_CHANNELS;

// A bit per channel, a kernel argument BY VALUE: the same for every lane, read through the scalar
// path.  (One word more than the channels need: col_bits_from reads two adjacent words.)
struct col_mask {
    uint32_t bits[COL_MAX_CHANNELS / 32 + 1];
};

__device__ inline float col_nan() { return __int_as_float(0x7fc00000); }

// Bit u of the result: channel c + u is in the mask, for u = 0 .. 32 -- one read of two adjacent words
// per round of the channel loop.  c is clamped so that the index stays in the mask whatever the
// caller's range; channels at and past `stop` are the caller's to mask out.
__device__ inline uint64_t col_bits_from(const col_mask &f, int c)
{
    c = min(max(c, 0), COL_MAX_CHANNELS - 1);
    const int i = c >> 5;
    return (((uint64_t) f.bits[i + 1] << 32) | f.bits[i]) >> (c & 31);
}

template <int V> __device__ inline void col_load(const float *p, float (&v)[V])
{
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = *p;
    }
}

template <int V, class T> __device__ inline void col_store(T *p, const T (&v)[V])
{
    if constexpr (V == 4) {
        struct alignas(16) quad { T a, b, c, d; };
        *reinterpret_cast<quad *>(p) = quad{v[0], v[1], v[2], v[3]};
    } else {
        *p = v[0];
    }
}

// The host's mask (one byte per channel, nonzero = in), packed
inline void col_set(col_mask &mask, int c) { mask.bits[c >> 5] |= 1u << (c & 31); }

// The form: four elements per thread where every address a thread forms is 16-byte aligned --
// `alignment` is the OR of every base address and of every pitch in bytes -- for the first
// 4 * (M / 4) elements, one element per thread for the tail and for everything else.  Returns how
// many elements the four-wide form takes (0: none).
inline int64_t col_vector_elements(uintptr_t alignment, int64_t plane_elements)
{
    if ((alignment & 15) == 0 && plane_elements >= 4)
        return plane_elements & ~(int64_t) 3;
    return 0;
}

// One thread per group of V elements: the plane a launch can cover, and its workgroups
inline bool col_plane_fits(int64_t plane_elements)
{
    return plane_elements <= (int64_t) 0x7fffffff * COL_THREADS;
}

inline unsigned col_blocks(int64_t groups) { return (unsigned) kimg_divup(groups, COL_THREADS); }

}  // namespace
