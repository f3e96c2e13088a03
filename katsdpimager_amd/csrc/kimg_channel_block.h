// What the per-channel operators on a raw [channel][row][pol] visibility block share (contsub.hip,
// statwt.hip, rfiflag.hip, spectral.hip, phaseshift.hip): the thread layout, the fit-channel mask,
// the load round, the group tables, the counters and the host's argument checks.  Only what at least
// two of the units use is here; moments.hip walks an image cube with a mask of its own and is no part
// of this.  Everything here is local to the including translation unit.
//
// The layout: one thread owns one element j of the dense [row][pol] plane and walks channels, so a
// wave reads 64 consecutive complex64 (512 B) and 64 consecutive weights (256 B) per channel, CB_UNROLL
// channels in flight together.  What is the same for every lane -- the mask, a basis, coefficients --
// is a kernel argument or read at a uniform address, and comes through the scalar path.
#pragma once
#include "kimg_common.h"

namespace {

constexpr int CB_THREADS = 256;
constexpr int CB_UNROLL = 4;                    // channels whose loads are in flight together
constexpr int CB_MAX_CHANNELS = KIMG_UVCONTSUB_MAX_CHANNELS;
constexpr int CB_MAX_BIN = KIMG_STATWT_MAX_BIN;     // rows of a group

// Element j of the plane, whether there is one, and the index a lane past the plane uses instead.
// A kernel with a wave-wide step (a ballot, a shuffle, __any) lets those lanes run along on `jj` and
// store nothing: its branches stay uniform and its counters are reduced over all 64 lanes.  A kernel
// without one returns on !live.  Which of the two is each kernel's own choice.
struct cb_lane {
    int64_t j, jj;
    bool live;
};

__device__ inline int64_t cb_element() { return (int64_t) blockIdx.x * CB_THREADS + threadIdx.x; }

__device__ inline cb_lane cb_lane_of(int64_t plane)
{
    cb_lane t;
    t.j = cb_element();
    t.live = t.j < plane;
    t.jj = t.live ? t.j : 0;
    return t;
}

// A bit per channel, passed to kernels BY VALUE as a kernel argument: the same for every lane, it is
// read through the scalar path, and a channel that is out is skipped by a uniform branch.
struct cb_mask {
    uint32_t bits[CB_MAX_CHANNELS / 32];
    __device__ bool operator[](int c) const { return (bits[c >> 5] >> (c & 31)) & 1u; }
};

// The host's mask (one byte per channel, nonzero = in) packed; returns how many channels are in.
// (Channels past CB_MAX_CHANNELS are counted and not packed: the caller turns such a band down.)
inline int64_t cb_pack_mask(const uint8_t *mask_host, int num_channels, cb_mask &mask)
{
    int64_t in = 0;
    mask = {};
    for (int c = 0; c < num_channels; c++)
        if (mask_host[c]) {
            in++;
            if (c < CB_MAX_CHANNELS)
                mask.bits[c >> 5] |= 1u << (c & 31);
        }
    return in;
}

// (v, w) of channels c0 .. c0 + CB_UNROLL - 1 of one lane, all loads issued before the first use;
// zeroes, and no load, where the channel is past C or not in the mask (fit[u] says which).  What a
// kernel adds up from them, and in which order, is the kernel's own: that is its contract.
__device__ __forceinline__ void cb_load_round(const float2 *v_ptr, int64_t vis_pitch,
                                              const float *w_ptr, int64_t weights_pitch, int C,
                                              const cb_mask &mask, int c0, float2 (&v)[CB_UNROLL],
                                              float (&w)[CB_UNROLL], bool (&fit)[CB_UNROLL])
{
#pragma unroll
    for (int u = 0; u < CB_UNROLL; u++) {
        const int c = c0 + u;
        fit[u] = c < C && mask[c];
        v[u] = make_float2(0.0f, 0.0f);
        w[u] = 0.0f;
        if (fit[u]) {
            v[u] = v_ptr[(int64_t) c * vis_pitch];
            w[u] = w_ptr[(int64_t) c * weights_pitch];
        }
    }
}

// Two, on purpose.  The continuum fit and the spectral filter take any positive weight, +inf included
// (their sums then become inf or NaN, which their contracts say what to do with); statwt and the
// flagger measure a scale from the weights themselves and leave a sample of infinite weight out.  The
// numpy twins say the same.
__device__ inline bool cb_usable(float w, float2 v)
{
    return w > 0.0f && isfinite(v.x) && isfinite(v.y);
}

__device__ inline bool cb_usable_finite_weight(float w, float2 v)
{
    return w > 0.0f && isfinite(w) && isfinite(v.x) && isfinite(v.y);
}

// Groups of up to CB_MAX_BIN consecutive rows of one baseline (statwt, the flagger)
struct cb_groups {
    const int32_t *offsets;     // [G + 1]
    const int32_t *row_group;   // [N]
    int G;
    int N;
    int P;
};

// Row and polarization of plane element j; the rows [r0, r1) of its group, and the group.  Whatever the
// tables hold, 0 <= g < G and 0 <= r0 <= r1 <= N with at most CB_MAX_BIN rows: nothing past the arrays
// is ever touched.  P_T: the number of polarizations where the kernel is a template of it, or 0 for
// "use the tables' value".
struct cb_place {
    int r, p, g, r0, r1;
};

template <int P_T = 0>
__device__ inline cb_place cb_place_of(const cb_groups &t, int64_t j)
{
    const int P = P_T ? P_T : t.P;
    cb_place at;
    at.r = (int) (j / P);
    at.p = (int) (j - (int64_t) at.r * P);
    at.g = min(max(t.row_group[at.r], 0), t.G - 1);
    at.r0 = min(max(t.offsets[at.g], 0), t.N);
    at.r1 = min(min(max(t.offsets[at.g + 1], at.r0), t.N), at.r0 + CB_MAX_BIN);
    return at;
}

// Two sums over the wave into counts[0] and counts[1], one atomic add each by the wave's first lane,
// none for a sum of zero.  All 64 lanes must be active.
__device__ inline void cb_add_nonzero(unsigned long long *counts, unsigned long long n0,
                                      unsigned long long n1)
{
    if (n0)
        atomicAdd(&counts[0], n0);
    if (n1)
        atomicAdd(&counts[1], n1);
}

// ... of two per-lane predicates
__device__ inline void cb_count_lanes(bool a, bool b, unsigned long long *counts)
{
    const unsigned long long n0 = __popcll(__ballot(a)), n1 = __popcll(__ballot(b));
    if ((threadIdx.x & (WAVE - 1)) == 0)
        cb_add_nonzero(counts, n0, n1);
}

__device__ inline unsigned long long cb_wave_sum(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_xor(v, off, WAVE);
    return (unsigned long long) v;
}

// ... of two per-lane integers
__device__ inline void cb_count_sums(int a, int b, unsigned long long *counts)
{
    const unsigned long long n0 = cb_wave_sum(a), n1 = cb_wave_sum(b);
    if ((threadIdx.x & (WAVE - 1)) == 0)
        cb_add_nonzero(counts, n0, n1);
}

// One thread per plane element: the plane a launch can cover, and its workgroups
inline bool cb_plane_fits(int64_t plane) { return plane <= (int64_t) 0x7fffffff * CB_THREADS; }

inline unsigned cb_blocks(int64_t plane) { return (unsigned) kimg_divup(plane, CB_THREADS); }

// The arguments of an entry point that works on a block in groups (kimg_statwt, kimg_rfi_flag), in
// the order of precedence of their contracts; `plane` = num_rows * num_pols once both are known to be
// in range.  The workspace must hold bytes_per_element per plane element and bytes_per_sample per
// sample.  Returns 0 with plane == 0 for a block without rows: there is nothing to do.  The caller
// checks the arguments of its own (all KIMG_EINVAL) ahead of this.
inline int cb_check_block(const void *vis, int64_t vis_channel_pitch, const float *weights,
                          int64_t weights_channel_pitch, int num_channels, int64_t num_rows,
                          int num_pols, const uint8_t *mask_host, const int32_t *group_offsets,
                          int64_t num_groups, const int32_t *row_group, int time_bin,
                          const void *workspace, size_t workspace_bytes, size_t bytes_per_element,
                          size_t bytes_per_sample, const uint64_t *counts, int64_t &plane)
{
    plane = 0;
    KIMG_CHECK_ARG(vis && weights && mask_host && group_offsets && row_group && workspace && counts);
    KIMG_CHECK_ARG(num_channels >= 1 && num_rows >= 0);
    KIMG_CHECK_ARG(num_pols >= 1 && num_pols <= 4);
    KIMG_CHECK_ARG(time_bin >= 1 && time_bin <= CB_MAX_BIN);
    // (rows are 32-bit in the group tables; the plane then stays far inside the grid limit)
    if (num_rows > 0x7fffffff)
        return KIMG_EUNSUPPORTED;
    const int64_t elements = num_rows * num_pols;
    KIMG_CHECK_ARG(vis_channel_pitch >= elements && weights_channel_pitch >= elements);
    if (num_channels > CB_MAX_CHANNELS)
        return KIMG_EUNSUPPORTED;
    if (elements == 0)
        return 0;
    KIMG_CHECK_ARG(num_groups >= 1 && num_groups <= num_rows && num_groups * time_bin >= num_rows);
    if (workspace_bytes < (size_t) elements * (bytes_per_element + (size_t) num_channels * bytes_per_sample))
        return KIMG_EWORKSPACE;
    KIMG_CHECK_ARG(((uintptr_t) workspace & 7) == 0);
    plane = elements;
    return 0;
}

}  // namespace
