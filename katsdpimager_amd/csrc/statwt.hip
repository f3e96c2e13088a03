// Statistical reweighting (include/kimg.h, "Statistical reweighting"): the weights of a
// [channel][row][pol] block of raw visibilities divided by the weighted scatter of the visibilities
// about their mean, taken per group of up to 64 consecutive rows of one baseline and per polarization
// across the line-free channels.  katsdpimager_amd/statwt.py holds the same contract as numpy
// (statwt_host), and the order of every sum below is that contract's: the device has the twin's bits.
//
// The thread layout, the fit mask, the load round and the group tables are kimg_channel_block.h's.
// Three launches, no LDS, no atomics on data, no cross-lane sums:
//   partials: (s0, sr, si, m) of the element's row over its usable fit channels -> workspace
//   scatter:  the element adds up the partials of its group's rows in ascending row order (every
//             element of a group does so for itself: at most 64 rows of 24 bytes, read through the
//             caches), forms the mean, walks the fit channels again and writes q of its row
//   apply:    the element adds up q and m of its group's rows, decides, and rescales or zeroes all its
//             channels; the first row of each group also writes chi2 and feeds the two counters (one
//             atomic add per wave each)
// Traffic per element: 12 bytes per fit channel twice, 8 per channel (4 where the group is flagged),
// 36 of workspace written and up to 64 x 36 read through the caches.
#include "kimg_channel_block.h"

namespace {

// The per-row partial sums between the launches, one entry per plane element each
struct sw_partials {
    double *s0, *sr, *si, *q;
    int *m;
};

__global__ __launch_bounds__(CB_THREADS)
void statwt_partials_kernel(const float2 *__restrict__ vis, int64_t vis_pitch,
                            const float *__restrict__ weights, int64_t weights_pitch, int C,
                            int64_t plane, const cb_mask mask, sw_partials out)
{
    // (lanes past the plane run along with clamped addresses and store nothing)
    const cb_lane t = cb_lane_of(plane);
    const float2 *v_ptr = vis + t.jj;
    const float *w_ptr = weights + t.jj;
    double s0 = 0.0, sr = 0.0, si = 0.0;
    int m = 0;
    for (int c0 = 0; c0 < C; c0 += CB_UNROLL) {
        float2 v[CB_UNROLL];
        float w[CB_UNROLL];
        bool fit[CB_UNROLL];
        cb_load_round(v_ptr, vis_pitch, w_ptr, weights_pitch, C, mask, c0, v, w, fit);
#pragma unroll
        for (int u = 0; u < CB_UNROLL; u++) {
            if (fit[u] && cb_usable_finite_weight(w[u], v[u])) {
                const double wd = (double) w[u];
                s0 += wd;
                sr += wd * (double) v[u].x;
                si += wd * (double) v[u].y;
                m++;
            }
        }
    }
    if (t.live) {
        out.s0[t.j] = s0;
        out.sr[t.j] = sr;
        out.si[t.j] = si;
        out.m[t.j] = m;
    }
}

template <int P>
__global__ __launch_bounds__(CB_THREADS)
void statwt_scatter_kernel(const float2 *__restrict__ vis, int64_t vis_pitch,
                           const float *__restrict__ weights, int64_t weights_pitch, int C,
                           int64_t plane, const cb_mask mask, cb_groups groups, sw_partials part)
{
    const cb_lane t = cb_lane_of(plane);
    const cb_place at = cb_place_of<P>(groups, t.jj);
    double S0 = 0.0, SR = 0.0, SI = 0.0;
    for (int rr = at.r0; rr < at.r1; rr++) {
        const int64_t k = (int64_t) rr * P + at.p;
        S0 += part.s0[k];
        SR += part.sr[k];
        SI += part.si[k];
    }
    const double mur = SR / S0, mui = SI / S0;

    const float2 *v_ptr = vis + t.jj;
    const float *w_ptr = weights + t.jj;
    double q = 0.0;
    for (int c0 = 0; c0 < C; c0 += CB_UNROLL) {
        float2 v[CB_UNROLL];
        float w[CB_UNROLL];
        bool fit[CB_UNROLL];
        cb_load_round(v_ptr, vis_pitch, w_ptr, weights_pitch, C, mask, c0, v, w, fit);
#pragma unroll
        for (int u = 0; u < CB_UNROLL; u++) {
            if (fit[u] && cb_usable_finite_weight(w[u], v[u])) {
                const double dr = (double) v[u].x - mur, di = (double) v[u].y - mui;
                double d2 = dr * dr;
                d2 = d2 + di * di;
                q += (double) w[u] * d2;
            }
        }
    }
    if (t.live)
        part.q[t.j] = q;
}

template <int P>
__global__ __launch_bounds__(CB_THREADS)
void statwt_apply_kernel(float *__restrict__ weights, int64_t weights_pitch, int C, int64_t plane,
                         cb_groups groups, sw_partials part, int min_samples, double lo, double hi,
                         double *__restrict__ chi2_out, unsigned long long *__restrict__ counts)
{
    const cb_lane t = cb_lane_of(plane);
    const bool live = t.live;
    const cb_place at = cb_place_of<P>(groups, t.jj);
    double Q = 0.0;
    int M = 0;
    for (int rr = at.r0; rr < at.r1; rr++) {
        const int64_t k = (int64_t) rr * P + at.p;
        Q += part.q[k];
        M += part.m[k];
    }
    const double chi2 = Q / (2.0 * (double) (M - 1));
    const bool kept = M >= min_samples && lo < chi2 && chi2 < hi;     // (false for a NaN)

    float *w_ptr = weights + t.jj;
    if (__any(live && kept)) {
        for (int c0 = 0; c0 < C; c0 += CB_UNROLL) {
            float w[CB_UNROLL];
#pragma unroll
            for (int u = 0; u < CB_UNROLL; u++) {
                w[u] = 0.0f;
                if (c0 + u < C && live && kept)
                    w[u] = w_ptr[(int64_t) (c0 + u) * weights_pitch];
            }
#pragma unroll
            for (int u = 0; u < CB_UNROLL; u++)
                if (c0 + u < C && live && kept && w[u] > 0.0f)
                    w_ptr[(int64_t) (c0 + u) * weights_pitch] = (float) ((double) w[u] / chi2);
        }
    }
    if (live && !kept)
        for (int c = 0; c < C; c++)
            w_ptr[(int64_t) c * weights_pitch] = 0.0f;

    const bool first = live && at.r == at.r0;
    if (first && chi2_out)
        chi2_out[(int64_t) at.g * P + at.p] =
            M < 2 ? __longlong_as_double(0x7ff8000000000000LL) : chi2;
    cb_count_lanes(first && kept, first && !kept, counts);
}

}  // namespace

extern "C" int kimg_statwt(const void *vis, int64_t vis_channel_pitch, float *weights,
                           int64_t weights_channel_pitch, int num_channels, int64_t num_rows,
                           int num_pols, const uint8_t *fit_mask_host, const int32_t *group_offsets,
                           int64_t num_groups, const int32_t *row_group, int time_bin,
                           int min_samples, double chi2_lo, double chi2_hi, double *chi2,
                           void *workspace, size_t workspace_bytes, uint64_t *counts, void *stream)
{
    KIMG_CHECK_ARG(min_samples >= 2);
    KIMG_CHECK_ARG(chi2_lo == chi2_lo && chi2_hi == chi2_hi);
    int64_t plane;
    const int rc = cb_check_block(vis, vis_channel_pitch, weights, weights_channel_pitch, num_channels,
                                  num_rows, num_pols, fit_mask_host, group_offsets, num_groups,
                                  row_group, time_bin, workspace, workspace_bytes,
                                  KIMG_STATWT_WORKSPACE_PER_ELEMENT, 0, counts, plane);
    if (rc != 0 || plane == 0)
        return rc;

    cb_mask mask;
    cb_pack_mask(fit_mask_host, num_channels, mask);
    sw_partials part;
    part.s0 = (double *) workspace;
    part.sr = part.s0 + plane;
    part.si = part.sr + plane;
    part.q = part.si + plane;
    part.m = (int *) (part.q + plane);
    const cb_groups groups = {group_offsets, row_group, (int) num_groups, (int) num_rows, num_pols};
    const float2 *v = (const float2 *) vis;
    hipStream_t s = (hipStream_t) stream;
    const unsigned blocks = cb_blocks(plane);
    statwt_partials_kernel<<<blocks, CB_THREADS, 0, s>>>(
        v, vis_channel_pitch, weights, weights_channel_pitch, num_channels, plane, mask, part);
    auto launch = [&](auto pols) {
        constexpr int P = decltype(pols)::value;
        statwt_scatter_kernel<P><<<blocks, CB_THREADS, 0, s>>>(
            v, vis_channel_pitch, weights, weights_channel_pitch, num_channels, plane, mask, groups, part);
        statwt_apply_kernel<P><<<blocks, CB_THREADS, 0, s>>>(
            weights, weights_channel_pitch, num_channels, plane, groups, part, min_samples, chi2_lo,
            chi2_hi, chi2, (unsigned long long *) counts);
    };
    kimg_for_pols(num_pols, launch);
    return kimg_launch_status();
}

KIMG_PRELOAD_THIS_UNIT(statwt_partials_kernel)
