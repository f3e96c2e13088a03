// Statistical reweighting (include/kimg.h, "Statistical reweighting"): the weights of a
// [channel][row][pol] block of raw visibilities divided by the weighted scatter of the visibilities
// about their mean, taken per group of up to 64 consecutive rows of one baseline and per polarization
// across the line-free channels.  katsdpimager_amd/statwt.py holds the same contract as numpy
// (statwt_host), and the order of every sum below is that contract's: the device has the twin's bits.
//
// The thread layout is contsub.hip's: one thread owns one element j of the dense [row][pol] plane and
// walks channels, so a wave reads 64 consecutive complex64 (512 B) and 64 consecutive weights (256 B)
// per channel; the fit mask (kernel argument, a bit per channel) is the same for every lane, so a line
// channel is skipped by a uniform branch.  Three launches, no LDS, no atomics on data, no cross-lane
// sums:
//   partials: (s0, sr, si, m) of the element's row over its usable fit channels -> workspace
//   scatter:  the element adds up the partials of its group's rows in ascending row order (every
//             element of a group does so for itself: at most 64 rows of 24 bytes, read through the
//             caches), forms the mean, walks the fit channels again and writes q of its row
//   apply:    the element adds up q and m of its group's rows, decides, and rescales or zeroes all its
//             channels; the first row of each group also writes chi2 and feeds the two counters (one
//             atomic add per wave each)
// Traffic per element: 12 bytes per fit channel twice, 8 per channel (4 where the group is flagged),
// 36 of workspace written and up to 64 x 36 read through the caches.
#include "kimg_common.h"

namespace {

constexpr int SW_THREADS = 256;
constexpr int SW_UNROLL = 4;                    // channels whose loads are in flight together
constexpr int SW_MAX_CHANNELS = KIMG_UVCONTSUB_MAX_CHANNELS;
constexpr int SW_MAX_BIN = KIMG_STATWT_MAX_BIN;

struct sw_mask {
    uint32_t bits[SW_MAX_CHANNELS / 32];
};

// The per-row partial sums between the launches, one entry per plane element each
struct sw_partials {
    double *s0, *sr, *si, *q;
    int *m;
};

struct sw_groups {
    const int32_t *offsets;     // [G + 1]
    const int32_t *row_group;   // [N]
    int G;
    int N;
};

__device__ inline bool sw_usable(float w, float2 v)
{
    return w > 0.0f && isfinite(w) && isfinite(v.x) && isfinite(v.y);
}

// The rows [r0, r1) of the group of row r, and the group.  Whatever the tables hold, 0 <= g < G and
// 0 <= r0 <= r1 <= N with at most SW_MAX_BIN rows: nothing past the arrays is ever touched.
__device__ inline void sw_group_of(const sw_groups &t, int r, int &g, int &r0, int &r1)
{
    g = min(max(t.row_group[r], 0), t.G - 1);
    r0 = min(max(t.offsets[g], 0), t.N);
    r1 = min(min(max(t.offsets[g + 1], r0), t.N), r0 + SW_MAX_BIN);
}

__global__ __launch_bounds__(SW_THREADS)
void statwt_partials_kernel(const float2 *__restrict__ vis, int64_t vis_pitch,
                            const float *__restrict__ weights, int64_t weights_pitch, int C,
                            int64_t plane, const sw_mask mask, sw_partials out)
{
    const int64_t j = (int64_t) blockIdx.x * SW_THREADS + threadIdx.x;
    const bool live = j < plane;
    // (lanes past the plane run along with clamped addresses and store nothing)
    const int64_t jj = live ? j : 0;
    const float2 *v_ptr = vis + jj;
    const float *w_ptr = weights + jj;
    double s0 = 0.0, sr = 0.0, si = 0.0;
    int m = 0;
    for (int c0 = 0; c0 < C; c0 += SW_UNROLL) {
        float2 v[SW_UNROLL];
        float w[SW_UNROLL];
        bool fit[SW_UNROLL];
#pragma unroll
        for (int u = 0; u < SW_UNROLL; u++) {
            const int c = c0 + u;
            fit[u] = c < C && ((mask.bits[c >> 5] >> (c & 31)) & 1u);
            v[u] = make_float2(0.0f, 0.0f);
            w[u] = 0.0f;
            if (fit[u]) {
                v[u] = v_ptr[(int64_t) c * vis_pitch];
                w[u] = w_ptr[(int64_t) c * weights_pitch];
            }
        }
#pragma unroll
        for (int u = 0; u < SW_UNROLL; u++) {
            if (fit[u] && sw_usable(w[u], v[u])) {
                const double wd = (double) w[u];
                s0 += wd;
                sr += wd * (double) v[u].x;
                si += wd * (double) v[u].y;
                m++;
            }
        }
    }
    if (live) {
        out.s0[j] = s0;
        out.sr[j] = sr;
        out.si[j] = si;
        out.m[j] = m;
    }
}

template <int P>
__global__ __launch_bounds__(SW_THREADS)
void statwt_scatter_kernel(const float2 *__restrict__ vis, int64_t vis_pitch,
                           const float *__restrict__ weights, int64_t weights_pitch, int C,
                           int64_t plane, const sw_mask mask, sw_groups groups, sw_partials part)
{
    const int64_t j = (int64_t) blockIdx.x * SW_THREADS + threadIdx.x;
    const bool live = j < plane;
    const int64_t jj = live ? j : 0;
    const int r = (int) (jj / P), p = (int) (jj - (int64_t) r * P);
    int g, r0, r1;
    sw_group_of(groups, r, g, r0, r1);
    double S0 = 0.0, SR = 0.0, SI = 0.0;
    for (int rr = r0; rr < r1; rr++) {
        const int64_t k = (int64_t) rr * P + p;
        S0 += part.s0[k];
        SR += part.sr[k];
        SI += part.si[k];
    }
    const double mur = SR / S0, mui = SI / S0;

    const float2 *v_ptr = vis + jj;
    const float *w_ptr = weights + jj;
    double q = 0.0;
    for (int c0 = 0; c0 < C; c0 += SW_UNROLL) {
        float2 v[SW_UNROLL];
        float w[SW_UNROLL];
        bool fit[SW_UNROLL];
#pragma unroll
        for (int u = 0; u < SW_UNROLL; u++) {
            const int c = c0 + u;
            fit[u] = c < C && ((mask.bits[c >> 5] >> (c & 31)) & 1u);
            v[u] = make_float2(0.0f, 0.0f);
            w[u] = 0.0f;
            if (fit[u]) {
                v[u] = v_ptr[(int64_t) c * vis_pitch];
                w[u] = w_ptr[(int64_t) c * weights_pitch];
            }
        }
#pragma unroll
        for (int u = 0; u < SW_UNROLL; u++) {
            if (fit[u] && sw_usable(w[u], v[u])) {
                const double dr = (double) v[u].x - mur, di = (double) v[u].y - mui;
                double t = dr * dr;
                t = t + di * di;
                q += (double) w[u] * t;
            }
        }
    }
    if (live)
        part.q[j] = q;
}

template <int P>
__global__ __launch_bounds__(SW_THREADS)
void statwt_apply_kernel(float *__restrict__ weights, int64_t weights_pitch, int C, int64_t plane,
                         sw_groups groups, sw_partials part, int min_samples, double lo, double hi,
                         double *__restrict__ chi2_out, unsigned long long *__restrict__ counts)
{
    const int64_t j = (int64_t) blockIdx.x * SW_THREADS + threadIdx.x;
    const bool live = j < plane;
    const int64_t jj = live ? j : 0;
    const int r = (int) (jj / P), p = (int) (jj - (int64_t) r * P);
    int g, r0, r1;
    sw_group_of(groups, r, g, r0, r1);
    double Q = 0.0;
    int M = 0;
    for (int rr = r0; rr < r1; rr++) {
        const int64_t k = (int64_t) rr * P + p;
        Q += part.q[k];
        M += part.m[k];
    }
    const double chi2 = Q / (2.0 * (double) (M - 1));
    const bool kept = M >= min_samples && lo < chi2 && chi2 < hi;     // (false for a NaN)

    float *w_ptr = weights + jj;
    if (__any(live && kept)) {
        for (int c0 = 0; c0 < C; c0 += SW_UNROLL) {
            float w[SW_UNROLL];
#pragma unroll
            for (int u = 0; u < SW_UNROLL; u++) {
                w[u] = 0.0f;
                if (c0 + u < C && live && kept)
                    w[u] = w_ptr[(int64_t) (c0 + u) * weights_pitch];
            }
#pragma unroll
            for (int u = 0; u < SW_UNROLL; u++)
                if (c0 + u < C && live && kept && w[u] > 0.0f)
                    w_ptr[(int64_t) (c0 + u) * weights_pitch] = (float) ((double) w[u] / chi2);
        }
    }
    if (live && !kept)
        for (int c = 0; c < C; c++)
            w_ptr[(int64_t) c * weights_pitch] = 0.0f;

    const bool first = live && r == r0;
    if (first && chi2_out)
        chi2_out[(int64_t) g * P + p] = M < 2 ? __longlong_as_double(0x7ff8000000000000LL) : chi2;
    const unsigned long long n_kept = __popcll(__ballot(first && kept));
    const unsigned long long n_flagged = __popcll(__ballot(first && !kept));
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        if (n_kept)
            atomicAdd(&counts[0], n_kept);
        if (n_flagged)
            atomicAdd(&counts[1], n_flagged);
    }
}

}  // namespace

extern "C" int kimg_statwt(const void *vis, int64_t vis_channel_pitch, float *weights,
                           int64_t weights_channel_pitch, int num_channels, int64_t num_rows,
                           int num_pols, const uint8_t *fit_mask_host, const int32_t *group_offsets,
                           int64_t num_groups, const int32_t *row_group, int time_bin,
                           int min_samples, double chi2_lo, double chi2_hi, double *chi2,
                           void *workspace, size_t workspace_bytes, uint64_t *counts, void *stream)
{
    KIMG_CHECK_ARG(vis && weights && fit_mask_host && group_offsets && row_group && workspace && counts);
    KIMG_CHECK_ARG(num_channels >= 1 && num_rows >= 0);
    KIMG_CHECK_ARG(num_pols >= 1 && num_pols <= 4);
    KIMG_CHECK_ARG(time_bin >= 1 && time_bin <= SW_MAX_BIN);
    KIMG_CHECK_ARG(min_samples >= 2);
    KIMG_CHECK_ARG(chi2_lo == chi2_lo && chi2_hi == chi2_hi);
    // (rows are 32-bit in the group tables; the plane then stays far inside the grid limit)
    if (num_rows > 0x7fffffff)
        return KIMG_EUNSUPPORTED;
    const int64_t plane = num_rows * num_pols;
    KIMG_CHECK_ARG(vis_channel_pitch >= plane && weights_channel_pitch >= plane);
    if (num_channels > SW_MAX_CHANNELS)
        return KIMG_EUNSUPPORTED;
    if (plane == 0)
        return 0;
    KIMG_CHECK_ARG(num_groups >= 1 && num_groups <= num_rows && num_groups * time_bin >= num_rows);
    if (workspace_bytes < (size_t) plane * KIMG_STATWT_WORKSPACE_PER_ELEMENT)
        return KIMG_EWORKSPACE;
    KIMG_CHECK_ARG(((uintptr_t) workspace & 7) == 0);

    sw_mask mask = {};
    for (int c = 0; c < num_channels; c++)
        if (fit_mask_host[c])
            mask.bits[c >> 5] |= 1u << (c & 31);
    sw_partials part;
    part.s0 = (double *) workspace;
    part.sr = part.s0 + plane;
    part.si = part.sr + plane;
    part.q = part.si + plane;
    part.m = (int *) (part.q + plane);
    const sw_groups groups = {group_offsets, row_group, (int) num_groups, (int) num_rows};
    const float2 *v = (const float2 *) vis;
    hipStream_t s = (hipStream_t) stream;
    const unsigned blocks = (unsigned) kimg_divup(plane, SW_THREADS);
    statwt_partials_kernel<<<blocks, SW_THREADS, 0, s>>>(
        v, vis_channel_pitch, weights, weights_channel_pitch, num_channels, plane, mask, part);
    auto launch = [&](auto pols) {
        constexpr int P = decltype(pols)::value;
        statwt_scatter_kernel<P><<<blocks, SW_THREADS, 0, s>>>(
            v, vis_channel_pitch, weights, weights_channel_pitch, num_channels, plane, mask, groups, part);
        statwt_apply_kernel<P><<<blocks, SW_THREADS, 0, s>>>(
            weights, weights_channel_pitch, num_channels, plane, groups, part, min_samples, chi2_lo,
            chi2_hi, chi2, (unsigned long long *) counts);
    };
    kimg_for_pols(num_pols, launch);
    return kimg_launch_status();
}

KIMG_PRELOAD_THIS_UNIT(statwt_partials_kernel)
