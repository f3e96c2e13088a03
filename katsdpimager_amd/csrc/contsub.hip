// UV-plane continuum subtraction (include/kimg.h, "UV-plane continuum subtraction"): a polynomial of
// order <= 3 fitted, per baseline sample, across the line-free channels of a [channel][row][pol]
// block of raw visibilities, and subtracted from every channel.  katsdpimager_amd/continuum.py holds
// the same contract as numpy (uvcontsub_host).
//
// One thread owns one element j of the dense [row][pol] plane, so a wave reads 64 consecutive
// complex64 (512 B) and 64 consecutive weights (256 B) per channel.  Pass 1 walks the fit channels and
// keeps the normal equations in registers (K (K + 1) / 2 + 2 K doubles, 18 at K = 4); the fit mask
// (kernel argument, a bit per channel) and the basis are the same for every lane, so a line channel is
// skipped by a uniform branch and the basis comes through the scalar cache.  The K x K system is
// solved in the thread.  Pass 2 walks every channel: read, subtract, store -- or, for a sample with
// fewer usable channels than coefficients, a zero into each of its weights.  No LDS, no atomics on
// data; the two counters take one atomic add per wave each.  Traffic per element: 12 bytes per fit
// channel, 16 per channel.
#include "kimg_common.h"

namespace {

constexpr int CS_THREADS = 256;
constexpr int CS_UNROLL = 4;                    // channels whose loads are in flight together
constexpr int CS_MAX_CHANNELS = KIMG_UVCONTSUB_MAX_CHANNELS;

struct cs_mask {
    uint32_t bits[CS_MAX_CHANNELS / 32];
};

template <int K>
__global__ __launch_bounds__(CS_THREADS)
void uvcontsub_kernel(float2 *__restrict__ vis, int64_t vis_pitch, float *__restrict__ weights,
                      int64_t weights_pitch, int C, int64_t plane, const cs_mask mask,
                      const double *__restrict__ basis, unsigned long long *__restrict__ counts)
{
    const int64_t j = (int64_t) blockIdx.x * CS_THREADS + threadIdx.x;
    const bool live = j < plane;
    // (lanes past the plane run along with clamped addresses and store nothing: the wave's branches
    // stay uniform and its counters are reduced over all 64 lanes)
    const int64_t jj = live ? j : 0;
    float2 *v_ptr = vis + jj;
    float *w_ptr = weights + jj;

    // A: lower triangle, row by row (A[k (k + 1) / 2 + l], l <= k)
    double A[K * (K + 1) / 2], br[K], bi[K];
#pragma unroll
    for (int i = 0; i < K * (K + 1) / 2; i++)
        A[i] = 0.0;
#pragma unroll
    for (int k = 0; k < K; k++)
        br[k] = bi[k] = 0.0;
    int m = 0;

    for (int c0 = 0; c0 < C; c0 += CS_UNROLL) {
        float2 v[CS_UNROLL];
        float w[CS_UNROLL];
        bool fit[CS_UNROLL];
#pragma unroll
        for (int u = 0; u < CS_UNROLL; u++) {
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
        for (int u = 0; u < CS_UNROLL; u++) {
            if (!fit[u])
                continue;
            const int c = c0 + u;
            const bool usable = w[u] > 0.0f && isfinite(v[u].x) && isfinite(v[u].y);
            if (usable) {
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
        // Cholesky A = L L^T in place, without pivoting, then L y = b and L^T a = y
#pragma unroll
        for (int k = 0; k < K; k++) {
#pragma unroll
            for (int l = 0; l <= k; l++) {
                double s = A[k * (k + 1) / 2 + l];
#pragma unroll
                for (int i = 0; i < l; i++)
                    s -= A[k * (k + 1) / 2 + i] * A[l * (l + 1) / 2 + i];
                A[k * (k + 1) / 2 + l] = l == k ? sqrt(s) : s / A[l * (l + 1) / 2 + l];
            }
        }
#pragma unroll
        for (int k = 0; k < K; k++) {
            double sr = br[k], si = bi[k];
#pragma unroll
            for (int i = 0; i < k; i++) {
                sr -= A[k * (k + 1) / 2 + i] * ar[i];
                si -= A[k * (k + 1) / 2 + i] * ai[i];
            }
            ar[k] = sr / A[k * (k + 1) / 2 + k];
            ai[k] = si / A[k * (k + 1) / 2 + k];
        }
#pragma unroll
        for (int k = K - 1; k >= 0; k--) {
            double sr = ar[k], si = ai[k];
#pragma unroll
            for (int i = k + 1; i < K; i++) {
                sr -= A[i * (i + 1) / 2 + k] * ar[i];
                si -= A[i * (i + 1) / 2 + k] * ai[i];
            }
            ar[k] = sr / A[k * (k + 1) / 2 + k];
            ai[k] = si / A[k * (k + 1) / 2 + k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < K; k++)
            ar[k] = ai[k] = 0.0;
    }

    if (__any(live && fitted)) {
        for (int c0 = 0; c0 < C; c0 += CS_UNROLL) {
            float2 v[CS_UNROLL];
#pragma unroll
            for (int u = 0; u < CS_UNROLL; u++)
                if (c0 + u < C)
                    v[u] = v_ptr[(int64_t) (c0 + u) * vis_pitch];
#pragma unroll
            for (int u = 0; u < CS_UNROLL; u++) {
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

    const unsigned long long n_fitted = __popcll(__ballot(live && fitted));
    const unsigned long long n_flagged = __popcll(__ballot(live && !fitted));
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        if (n_fitted)
            atomicAdd(&counts[0], n_fitted);
        if (n_flagged)
            atomicAdd(&counts[1], n_flagged);
    }
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
    int64_t fit_channels = 0;
    for (int c = 0; c < num_channels; c++)
        fit_channels += fit_mask_host[c] != 0;
    if (K > fit_channels || num_channels > CS_MAX_CHANNELS)
        return KIMG_EUNSUPPORTED;
    KIMG_CHECK_ARG(vis && weights && basis && counts && plane_elements >= 0);
    KIMG_CHECK_ARG(vis_channel_pitch >= plane_elements && weights_channel_pitch >= plane_elements);
    if (plane_elements > (int64_t) 0x7fffffff * CS_THREADS)
        return KIMG_EUNSUPPORTED;
    if (plane_elements == 0)
        return 0;
    cs_mask mask = {};
    for (int c = 0; c < num_channels; c++)
        if (fit_mask_host[c])
            mask.bits[c >> 5] |= 1u << (c & 31);
    hipStream_t s = (hipStream_t) stream;
    const unsigned blocks = (unsigned) kimg_divup(plane_elements, CS_THREADS);
    auto launch = [&](auto k) {
        uvcontsub_kernel<decltype(k)::value><<<blocks, CS_THREADS, 0, s>>>(
            (float2 *) vis, vis_channel_pitch, weights, weights_channel_pitch, num_channels,
            plane_elements, mask, basis, (unsigned long long *) counts);
    };
    kimg_for_pols(K, launch);       // (K is 1 .. 4, like a polarization count)
    return kimg_launch_status();
}

KIMG_PRELOAD_THIS_UNIT(uvcontsub_kernel<1>)
