// UV-plane continuum subtraction (include/kimg.h, "UV-plane continuum subtraction"): a polynomial of
// order <= 3 fitted, per baseline sample, across the line-free channels of a [channel][row][pol]
// block of raw visibilities, and subtracted from every channel.  katsdpimager_amd/continuum.py holds
// the same contract as numpy (uvcontsub_host).
//
// The thread layout, the fit mask and the load round are kimg_channel_block.h's.  Pass 1 walks the fit
// channels and keeps the normal equations in registers (K (K + 1) / 2 + 2 K doubles, 18 at K = 4); the
// basis is the same for every lane and comes through the scalar cache.  The K x K system is
// solved in the thread (kimg_cholesky.h, shared with imcontsub.hip).  Pass 2 walks every channel: read, subtract, store -- or, for a sample with
// fewer usable channels than coefficients, a zero into each of its weights.  No LDS, no atomics on
// data; the two counters take one atomic add per wave each.  Traffic per element: 12 bytes per fit
// channel, 16 per channel.
#include "kimg_channel_block.h"
#include "kimg_cholesky.h"

namespace {

template <int K>
__global__ __launch_bounds__(CB_THREADS)
void uvcontsub_kernel(float2 *__restrict__ vis, int64_t vis_pitch, float *__restrict__ weights,
                      int64_t weights_pitch, int C, int64_t plane, const cb_mask mask,
                      const double *__restrict__ basis, unsigned long long *__restrict__ counts)
{
    // (lanes past the plane run along: the __any and the counters below are wave-wide)
    const cb_lane t = cb_lane_of(plane);
    const bool live = t.live;
    float2 *v_ptr = vis + t.jj;
    float *w_ptr = weights + t.jj;

    // A: lower triangle, row by row (A[k (k + 1) / 2 + l], l <= k)
    double A[K * (K + 1) / 2], br[K], bi[K];
#pragma unroll
    for (int i = 0; i < K * (K + 1) / 2; i++)
        A[i] = 0.0;
#pragma unroll
    for (int k = 0; k < K; k++)
        br[k] = bi[k] = 0.0;
    int m = 0;

    for (int c0 = 0; c0 < C; c0 += CB_UNROLL) {
        float2 v[CB_UNROLL];
        float w[CB_UNROLL];
        bool fit[CB_UNROLL];
        cb_load_round(v_ptr, vis_pitch, w_ptr, weights_pitch, C, mask, c0, v, w, fit);
#pragma unroll
        for (int u = 0; u < CB_UNROLL; u++) {
            if (!fit[u])
                continue;
            const int c = c0 + u;
            if (cb_usable(w[u], v[u])) {
                m++;
                const double wd = (double) w[u], vr = (double) v[u].x, vi = (double) v[u].y;
#pragma unroll
                for (int k = 0; k < K; k++) {
                    const double wb = wd * basis[(int64_t) k * C + c];
#pragma unroll
                    for (int l = 0; l <= k; l++)
                        A[k * (k + 1) / 2 + l] += wb * basis[(int64_t) l * C + c];
                    br[k] += wb * vr;
                    bi[k] += wb * vi;
                }
            }
        }
    }

    const bool fitted = m >= K;
    double ar[K], ai[K];
    if (fitted) {
        // Cholesky A = L L^T in place, without pivoting, then L y = b and L^T a = y for either part
        kimg_cholesky<K>(A);
        kimg_cholesky_solve<K>(A, br, ar);
        kimg_cholesky_solve<K>(A, bi, ai);
    } else {
#pragma unroll
        for (int k = 0; k < K; k++)
            ar[k] = ai[k] = 0.0;
    }

    if (__any(live && fitted)) {
        for (int c0 = 0; c0 < C; c0 += CB_UNROLL) {
            float2 v[CB_UNROLL];
#pragma unroll
            for (int u = 0; u < CB_UNROLL; u++)
                if (c0 + u < C)
                    v[u] = v_ptr[(int64_t) (c0 + u) * vis_pitch];
#pragma unroll
            for (int u = 0; u < CB_UNROLL; u++) {
                const int c = c0 + u;
                if (c >= C)
                    continue;
                double mr = 0.0, mi = 0.0;
#pragma unroll
                for (int k = 0; k < K; k++) {
                    const double b = basis[(int64_t) k * C + c];
                    mr += ar[k] * b;
                    mi += ai[k] * b;
                }
                if (live && fitted)
                    v_ptr[(int64_t) c * vis_pitch] =
                        make_float2((float) ((double) v[u].x - mr), (float) ((double) v[u].y - mi));
            }
        }
    }
    if (live && !fitted)
        for (int c = 0; c < C; c++)
            w_ptr[(int64_t) c * weights_pitch] = 0.0f;

    cb_count_lanes(live && fitted, live && !fitted, counts);
}

}  // namespace

extern "C" int kimg_uvcontsub(void *vis, int64_t vis_channel_pitch, float *weights,
                              int64_t weights_channel_pitch, int num_channels,
                              int64_t plane_elements, const uint8_t *fit_mask_host,
                              const double *basis, int order, uint64_t *counts, void *stream)
{
    KIMG_CHECK_ARG(order >= 0 && order <= KIMG_UVCONTSUB_MAX_ORDER && num_channels >= 1);
    KIMG_CHECK_ARG(fit_mask_host);
    const int K = order + 1;
    cb_mask mask;
    const int64_t fit_channels = cb_pack_mask(fit_mask_host, num_channels, mask);
    if (K > fit_channels || num_channels > CB_MAX_CHANNELS)
        return KIMG_EUNSUPPORTED;
    KIMG_CHECK_ARG(vis && weights && basis && counts && plane_elements >= 0);
    KIMG_CHECK_ARG(vis_channel_pitch >= plane_elements && weights_channel_pitch >= plane_elements);
    if (!cb_plane_fits(plane_elements))
        return KIMG_EUNSUPPORTED;
    if (plane_elements == 0)
        return 0;
    hipStream_t s = (hipStream_t) stream;
    const unsigned blocks = cb_blocks(plane_elements);
    auto launch = [&](auto k) {
        uvcontsub_kernel<decltype(k)::value><<<blocks, CB_THREADS, 0, s>>>(
            (float2 *) vis, vis_channel_pitch, weights, weights_channel_pitch, num_channels,
            plane_elements, mask, basis, (unsigned long long *) counts);
    };
    kimg_for_pols(K, launch);       // (K is 1 .. 4, like a polarization count)
    return kimg_launch_status();
}

KIMG_PRELOAD_THIS_UNIT(uvcontsub_kernel<1>)
