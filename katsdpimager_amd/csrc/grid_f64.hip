// Float64 gridder and degridder (the reference's --precision double, frontend.py:300): the grid is
// complex128; visibilities and the kernel table stay complex64, weights float32 (the reference's
// types, grid.py:536-539, :686-690).  Arithmetic contract: include/kimg.h, kimg_grid_f64.
//
// Widths up to 32: a moving 32 x 32 window of the grid held in registers (below; KIMG_VARIANT_MFMA,
// and AUTO), also run over tile-sorted copies of the stream (KIMG_VARIANT_BINNED, grid_binned.hip).
// Any width: the generic kernels, one wave per visibility, lanes over the K x K footprint (lane % 32
// along u, so that a half-wave's atomics cover 32 contiguous complex128 cells of one grid row); every
// tap of the generic gridder is a pair of global_atomic_add_f64 (-munsafe-fp-atomics: no CAS loop).
// Widths 33..64 do not take the float32 kernel's 2 x 2 tap-block split: they run the generic kernels.
#include "kimg_common.h"

namespace {

// a * b in double, the two products of each part rounded separately (like numpy's complex128
// multiply; the library is built with -ffp-contract=off)
__device__ inline double2 zmul(double2 a, double2 b)
{
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

__device__ inline double2 widen(float2 a) { return make_double2((double) a.x, (double) a.y); }

__device__ inline double2 widen_conj(float2 a) { return make_double2((double) a.x, -(double) a.y); }

// grid[p][v0+j][u0+k] += (s_p * conj(kv_j)) * conj(ku_k), s_p = float32(vis_p * wgt_p)
template <int P>
__global__ __launch_bounds__(256) void grid_f64_generic_kernel(
    double *__restrict__ grid, int64_t row_stride, int64_t pol_stride, int Gg,
    const float *__restrict__ weights_grid, int64_t wg_row_stride, int64_t wg_pol_stride,
    const int16_t *__restrict__ uv, const int16_t *__restrict__ w_plane,
    const float2 *__restrict__ vis, int64_t num_vis,
    const float2 *__restrict__ kern, int w_planes, int oversample, int K)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t) blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t) gridDim.x * (blockDim.x >> 6);
    const int half = Gg / 2;
    const int uv_bias = (K - 1) / 2 - half;                     // grid.py:1038
    for (int64_t i = wave; i < num_vis; i += nwaves) {
        const vis_coord c = load_uv(uv, i);
        const int wp = w_plane[i];
        if (!coords_ok(c, wp, Gg, w_planes, oversample))
            continue;                                           // (uniform over the wave)
        const int u0 = c.u - uv_bias, v0 = c.v - uv_bias;
        const int64_t wa = (int64_t) (c.v + half) * wg_row_stride + (c.u + half);
        double2 sample[P];
#pragma unroll
        for (int p = 0; p < P; p++) {
            const float wgt = weights_grid[wa + p * wg_pol_stride];
            const float2 s = vis[i * P + p];
            sample[p] = make_double2((double) (s.x * wgt), (double) (s.y * wgt));
        }
        const float2 *kv = kern + ((int64_t) wp * oversample + c.sub_v) * K;
        const float2 *ku = kern + ((int64_t) wp * oversample + c.sub_u) * K;
        for (int k = lane & 31; k < K; k += 32) {
            const int x = u0 + k;
            if ((unsigned) x >= (unsigned) Gg)
                continue;
            const double2 wu = widen_conj(ku[k]);
            for (int j = lane >> 5; j < K; j += 2) {
                const int y = v0 + j;
                if ((unsigned) y >= (unsigned) Gg)
                    continue;
                const double2 wv = widen_conj(kv[j]);
                const int64_t a = 2 * ((int64_t) y * row_stride + x);
#pragma unroll
                for (int p = 0; p < P; p++) {
                    const double2 upd = zmul(zmul(sample[p], wv), wu);
                    atomicAdd(&grid[a + 2 * p * pol_stride], upd.x);
                    atomicAdd(&grid[a + 2 * p * pol_stride + 1], upd.y);
                }
            }
        }
    }
}

// vis[p] = complex64(vis[p] - weight[p] * sum_k ku_k sum_j kv_j grid[p][v0+j][u0+k]), in double
template <int P>
__global__ __launch_bounds__(256) void degrid_f64_generic_kernel(
    const double2 *__restrict__ grid, int64_t row_stride, int64_t pol_stride, int Gg,
    const int16_t *__restrict__ uv, const int16_t *__restrict__ w_plane,
    const float *__restrict__ weights, float2 *__restrict__ vis, int64_t num_vis,
    const float2 *__restrict__ kern, int w_planes, int oversample, int K)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t) blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t) gridDim.x * (blockDim.x >> 6);
    const int uv_bias = (K - 1) / 2 - Gg / 2;                   // grid.py:1141
    for (int64_t i = wave; i < num_vis; i += nwaves) {
        const vis_coord c = load_uv(uv, i);
        const int wp = w_plane[i];
        if (!coords_ok(c, wp, Gg, w_planes, oversample))
            continue;                                           // predicts 0: vis unchanged
        const int u0 = c.u - uv_bias, v0 = c.v - uv_bias;
        const float2 *kv = kern + ((int64_t) wp * oversample + c.sub_v) * K;
        const float2 *ku = kern + ((int64_t) wp * oversample + c.sub_u) * K;
        double2 acc[P];
#pragma unroll
        for (int p = 0; p < P; p++)
            acc[p] = make_double2(0.0, 0.0);
        for (int k = lane & 31; k < K; k += 32) {
            const int x = u0 + k;
            if ((unsigned) x >= (unsigned) Gg)
                continue;
            const double2 wu = widen(ku[k]);
            double2 t[P];
#pragma unroll
            for (int p = 0; p < P; p++)
                t[p] = make_double2(0.0, 0.0);
            for (int j = lane >> 5; j < K; j += 2) {
                const int y = v0 + j;
                if ((unsigned) y >= (unsigned) Gg)
                    continue;
                const double2 wv = widen(kv[j]);
                const int64_t a = (int64_t) y * row_stride + x;
#pragma unroll
                for (int p = 0; p < P; p++) {
                    const double2 prod = zmul(wv, grid[a + p * pol_stride]);
                    t[p].x += prod.x;
                    t[p].y += prod.y;
                }
            }
#pragma unroll
            for (int p = 0; p < P; p++) {
                const double2 prod = zmul(wu, t[p]);
                acc[p].x += prod.x;
                acc[p].y += prod.y;
            }
        }
#pragma unroll
        for (int p = 0; p < P; p++) {
            acc[p].x = wave_sum(acc[p].x);
            acc[p].y = wave_sum(acc[p].y);
        }
        if (lane < P) {
            double2 a = acc[0];
#pragma unroll
            for (int p = 1; p < P; p++)
                if (lane == p)
                    a = acc[p];
            const double wgt = weights[i * P + lane];
            const float2 old = vis[i * P + lane];
            // one rounding: DegridderHost._degrid with complex128 values (grid.py:1139-1154)
            vis[i * P + lane] = make_float2((float) ((double) old.x - wgt * a.x),
                                            (float) ((double) old.y - wgt * a.y));
        }
    }
}

// ---- window kernels (widths <= 32) ---------------------------------------------------------------
// A wave (one 64-thread workgroup) owns one polarization of a contiguous chunk of the stream and a
// 32 x 32 complex128 window of the grid in registers: lane l holds column c = l & 31 and rows
// r = (l >> 5) + 2 i, i = 0..15 (16 complex cells, 64 VGPRs).  Cell (r, c) stands for grid point
// (Wv + ((r - Wv) & 31), Wu + ((c - Wu) & 31)), so the window slides without moving data.  A record
// whose footprint leaves the window moves the origin as little as needed (slack 32 - K), and only
// the cells whose mapping changes are flushed with global_atomic_add_f64: a half-wave's flush is
// one grid row of 32 contiguous complex128 cells.  Per record each lane does 16 complex FMAs on the
// VALU (v_fma_f64: see DESIGN 5.8 for the MFMA / VALU measurement), reading the row factor
// a_j = s conj(kv_j) from LDS and its own column tap.  One polarization per wave keeps the window
// at 64 VGPRs for any P.
constexpr int WINF = 32;

__device__ inline double2 zfma(double2 a, double2 b, double2 c)
{
    return make_double2(fma(a.x, b.x, fma(-a.y, b.y, c.x)), fma(a.x, b.y, fma(a.y, b.x, c.y)));
}

// new window origin along one axis for a footprint [x0, x0 + K): the least move that covers it
__device__ inline int window_origin(bool have, int W, int x0, int K)
{
    if (!have)
        return x0;
    if (x0 < W)
        return x0;
    if (x0 + K > W + WINF)
        return x0 + K - WINF;
    return W;
}

template <int P>
__global__ __launch_bounds__(64) void grid_f64_window_kernel(
    double *__restrict__ grid, int64_t row_stride, int64_t pol_stride, int Gg,
    const float *__restrict__ weights_grid, int64_t wg_row_stride, int64_t wg_pol_stride,
    const int16_t *__restrict__ uv, const int16_t *__restrict__ w_plane,
    const float2 *__restrict__ vis, int64_t num_vis,
    const float2 *__restrict__ kern, int w_planes, int oversample, int K, int64_t chunk)
{
    __shared__ double2 arow[WINF];
    const int lane = threadIdx.x;
    const int p = blockIdx.y;
    const int64_t begin = (int64_t) blockIdx.x * chunk;
    const int64_t end = begin + chunk < num_vis ? begin + chunk : num_vis;
    const int c = lane & 31, h = lane >> 5;
    const int half = Gg / 2;
    const int uv_bias = (K - 1) / 2 - half;                     // grid.py:1038
    double *const g = grid + 2 * p * pol_stride;
    double2 acc[16];
#pragma unroll
    for (int i = 0; i < 16; i++)
        acc[i] = make_double2(0.0, 0.0);
    bool have = false;
    int Wu = 0, Wv = 0;

    // add and clear every cell whose mapping differs between origins (Wu, Wv) and (nWu, nWv)
    auto flush = [&](int nWu, int nWv, bool all) __attribute__((always_inline)) {
        const int x = Wu + ((c - Wu) & 31);
        const bool col = all || x != nWu + ((c - nWu) & 31);
        const bool x_in = (unsigned) x < (unsigned) Gg;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int r = h + 2 * i;
            const int y = Wv + ((r - Wv) & 31);
            if (col || y != nWv + ((r - nWv) & 31)) {
                if (x_in && (unsigned) y < (unsigned) Gg
                    && (acc[i].x != 0.0 || acc[i].y != 0.0)) {
                    double *cell = g + 2 * ((int64_t) y * row_stride + x);
                    atomicAdd(cell, acc[i].x);
                    atomicAdd(cell + 1, acc[i].y);
                }
                acc[i] = make_double2(0.0, 0.0);
            }
        }
    };

    for (int64_t i = begin; i < end; i++) {
        const vis_coord co = load_uv(uv, i);
        const int wp = w_plane[i];
        if (!coords_ok(co, wp, Gg, w_planes, oversample))
            continue;                                           // (uniform over the wave)
        const int x0 = co.u - uv_bias, y0 = co.v - uv_bias;
        if (!have || x0 < Wu || x0 + K > Wu + WINF || y0 < Wv || y0 + K > Wv + WINF) {
            const int nWu = window_origin(have, Wu, x0, K), nWv = window_origin(have, Wv, y0, K);
            if (have)
                flush(nWu, nWv, false);
            Wu = nWu;
            Wv = nWv;
            have = true;
        }
        const float wgt = weights_grid[(int64_t) (co.v + half) * wg_row_stride + (co.u + half)
                                       + p * wg_pol_stride];
        const float2 sv = vis[i * P + p];
        const double2 s = make_double2((double) (sv.x * wgt), (double) (sv.y * wgt));
        const float2 *kv = kern + ((int64_t) wp * oversample + co.sub_v) * K;
        const float2 *ku = kern + ((int64_t) wp * oversample + co.sub_u) * K;
        if (lane < WINF)
            arow[lane] = lane < K ? zmul(s, widen_conj(kv[lane])) : make_double2(0.0, 0.0);
        const int k = (c - x0) & 31;
        const double2 b = k < K ? widen_conj(ku[k]) : make_double2(0.0, 0.0);
        __syncthreads();
#pragma unroll
        for (int r_i = 0; r_i < 16; r_i++) {
            const int j = (h + 2 * r_i - y0) & 31;
            acc[r_i] = zfma(arow[j], b, acc[r_i]);
        }
        __syncthreads();
    }
    if (have)
        flush(Wu, Wv, true);
}

// Degridder on the same window: the cells of the grid in registers, (re)loaded only where the
// mapping changes; per record each lane forms t = sum over its 16 rows of kv_j g[j][k], then
// ku_k t, summed over the wave.
template <int P>
__global__ __launch_bounds__(64) void degrid_f64_window_kernel(
    const double2 *__restrict__ grid, int64_t row_stride, int64_t pol_stride, int Gg,
    const int16_t *__restrict__ uv, const int16_t *__restrict__ w_plane,
    const float *__restrict__ weights, float2 *__restrict__ vis, int64_t num_vis,
    const float2 *__restrict__ kern, int w_planes, int oversample, int K, int64_t chunk)
{
    __shared__ double2 krow[WINF];
    const int lane = threadIdx.x;
    const int p = blockIdx.y;
    const int64_t begin = (int64_t) blockIdx.x * chunk;
    const int64_t end = begin + chunk < num_vis ? begin + chunk : num_vis;
    const int c = lane & 31, h = lane >> 5;
    const int uv_bias = (K - 1) / 2 - Gg / 2;                   // grid.py:1141
    const double2 *const g = grid + p * pol_stride;
    double2 win[16];
    bool have = false;
    int Wu = 0, Wv = 0;

    // load every cell whose mapping differs between the old origin and (nWu, nWv)
    auto refill = [&](int nWu, int nWv, bool all) __attribute__((always_inline)) {
        const int x = nWu + ((c - nWu) & 31);
        const bool col = all || x != Wu + ((c - Wu) & 31);
        const bool x_in = (unsigned) x < (unsigned) Gg;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int r = h + 2 * i;
            const int y = nWv + ((r - nWv) & 31);
            if (col || y != Wv + ((r - Wv) & 31))
                win[i] = x_in && (unsigned) y < (unsigned) Gg ? g[(int64_t) y * row_stride + x]
                                                               : make_double2(0.0, 0.0);
        }
    };

    for (int64_t i = begin; i < end; i++) {
        const vis_coord co = load_uv(uv, i);
        const int wp = w_plane[i];
        if (!coords_ok(co, wp, Gg, w_planes, oversample))
            continue;                                           // predicts 0: vis unchanged
        const int x0 = co.u - uv_bias, y0 = co.v - uv_bias;
        if (!have || x0 < Wu || x0 + K > Wu + WINF || y0 < Wv || y0 + K > Wv + WINF) {
            const int nWu = window_origin(have, Wu, x0, K), nWv = window_origin(have, Wv, y0, K);
            refill(nWu, nWv, !have);
            Wu = nWu;
            Wv = nWv;
            have = true;
        }
        const float2 *kv = kern + ((int64_t) wp * oversample + co.sub_v) * K;
        const float2 *ku = kern + ((int64_t) wp * oversample + co.sub_u) * K;
        if (lane < WINF)
            krow[lane] = lane < K ? widen(kv[lane]) : make_double2(0.0, 0.0);
        const int k = (c - x0) & 31;
        const double2 b = k < K ? widen(ku[k]) : make_double2(0.0, 0.0);
        __syncthreads();
        double2 t = make_double2(0.0, 0.0);
#pragma unroll
        for (int r_i = 0; r_i < 16; r_i++)
            t = zfma(krow[(h + 2 * r_i - y0) & 31], win[r_i], t);
        const double2 bt = zmul(b, t);
        const double px = wave_sum(bt.x), py = wave_sum(bt.y);
        if (lane == 0) {
            const double wgt = weights[i * P + p];
            const float2 old = vis[i * P + p];
            vis[i * P + p] = make_float2((float) ((double) old.x - wgt * px),
                                         (float) ((double) old.y - wgt * py));
        }
        __syncthreads();
    }
}

// chunk of the stream per wave: enough waves to fill the chip, enough records per wave for the
// window to pay
int64_t window_chunk(int64_t num_vis, int P)
{
    const int64_t waves = 4096 / P;
    int64_t chunk = (num_vis + waves - 1) / waves;
    return chunk < 256 ? 256 : chunk;
}

int check_f64_args(int grid_size, int P, int64_t num_vis, int w_planes, int oversample, int K,
                   int variant)
{
    if (grid_size <= 0 || grid_size % 2 || num_vis < 0 || w_planes <= 0 || oversample <= 0
        || K <= 0 || K > grid_size || variant < 0 || (variant >> 8) > 256)
        return KIMG_EINVAL;
    variant &= 0xff;
    if (variant != KIMG_VARIANT_AUTO && variant != KIMG_VARIANT_GENERIC
        && variant != KIMG_VARIANT_MFMA && variant != KIMG_VARIANT_BINNED)
        return KIMG_EINVAL;
    if (P < 1 || P > 4)
        return KIMG_EUNSUPPORTED;
    if ((variant == KIMG_VARIANT_MFMA || variant == KIMG_VARIANT_BINNED) && K > WINF)
        return KIMG_EUNSUPPORTED;                               // widths 33..: generic only
    return 0;
}

} // namespace

// the window kernels over a stream as given
int kimg_grid_window_f64(double *grid, int64_t grid_row_stride, int64_t grid_pol_stride,
                         int grid_size, int P, const float *weights_grid, int64_t wg_row_stride,
                         int64_t wg_pol_stride, const int16_t *uv, const int16_t *w_plane,
                         const float2 *vis, int64_t num_vis, const float2 *kern, int w_planes,
                         int oversample, int K, hipStream_t s)
{
    const int64_t chunk = window_chunk(num_vis, P);
    const dim3 blocks(kimg_divup(num_vis, chunk), P);
    kimg_for_pols(P, [&](auto p) {
        grid_f64_window_kernel<decltype(p)::value><<<blocks, 64, 0, s>>>(
            grid, grid_row_stride, grid_pol_stride, grid_size, weights_grid, wg_row_stride,
            wg_pol_stride, uv, w_plane, vis, num_vis, kern, w_planes, oversample, K, chunk); });
    return kimg_launch_status();
}

int kimg_degrid_window_f64(const double2 *grid, int64_t grid_row_stride, int64_t grid_pol_stride,
                           int grid_size, int P, const int16_t *uv, const int16_t *w_plane,
                           const float *weights, float2 *vis, int64_t num_vis, const float2 *kern,
                           int w_planes, int oversample, int K, hipStream_t s)
{
    const int64_t chunk = window_chunk(num_vis, P);
    const dim3 blocks(kimg_divup(num_vis, chunk), P);
    kimg_for_pols(P, [&](auto p) {
        degrid_f64_window_kernel<decltype(p)::value><<<blocks, 64, 0, s>>>(
            grid, grid_row_stride, grid_pol_stride, grid_size, uv, w_plane, weights, vis, num_vis,
            kern, w_planes, oversample, K, chunk); });
    return kimg_launch_status();
}

extern "C" int kimg_grid_f64(void *grid, int64_t grid_row_stride, int64_t grid_pol_stride,
                             int grid_size, int num_polarizations, const float *weights_grid,
                             int64_t wg_row_stride, int64_t wg_pol_stride, const int16_t *uv,
                             const int16_t *w_plane, const void *vis, int64_t num_vis,
                             const void *convolve_kernel, int w_planes, int oversample,
                             int kernel_width, void *workspace, size_t workspace_bytes,
                             int variant, void *stream)
{
    KIMG_CHECK_ARG(grid && weights_grid && uv && w_plane && vis && convolve_kernel);
    KIMG_CHECK_ARG(grid_row_stride >= grid_size && wg_row_stride >= grid_size);
    int rc = check_f64_args(grid_size, num_polarizations, num_vis, w_planes, oversample,
                            kernel_width, variant);
    if (rc)
        return rc;
    if (num_vis == 0)
        return 0;
    variant &= 0xff;
    hipStream_t s = (hipStream_t) stream;
    if (variant == KIMG_VARIANT_BINNED) {
        // the float32 path's sort and gather into the same scratch (of which the padded-table part
        // goes unused), then the window kernel on the sorted copies
        kimg_binned_stream b;
        rc = kimg_bin_stream(uv, w_plane, nullptr, vis, num_vis, grid_size, num_polarizations,
                             w_planes, oversample, kernel_width, workspace, workspace_bytes, s, b);
        if (rc)
            return rc;
        return kimg_grid_window_f64((double *) grid, grid_row_stride, grid_pol_stride, grid_size,
                                    num_polarizations, weights_grid, wg_row_stride, wg_pol_stride,
                                    b.uv, b.w_plane, b.vis, num_vis,
                                    (const float2 *) convolve_kernel, w_planes, oversample,
                                    kernel_width, s);
    }
    if (variant == KIMG_VARIANT_MFMA || (variant == KIMG_VARIANT_AUTO && kernel_width <= WINF))
        return kimg_grid_window_f64((double *) grid, grid_row_stride, grid_pol_stride, grid_size,
                                    num_polarizations, weights_grid, wg_row_stride, wg_pol_stride,
                                    uv, w_plane, (const float2 *) vis, num_vis,
                                    (const float2 *) convolve_kernel, w_planes, oversample,
                                    kernel_width, s);
    int blocks = kimg_divup(num_vis, 4);
    if (blocks > 8192)
        blocks = 8192;
    kimg_for_pols(num_polarizations, [&](auto p) {
        grid_f64_generic_kernel<decltype(p)::value><<<blocks, 256, 0, s>>>(
            (double *) grid, grid_row_stride, grid_pol_stride, grid_size, weights_grid, wg_row_stride,
            wg_pol_stride, uv, w_plane, (const float2 *) vis, num_vis,
            (const float2 *) convolve_kernel, w_planes, oversample, kernel_width); });
    return kimg_launch_status();
}

extern "C" int kimg_degrid_f64(const void *grid, int64_t grid_row_stride, int64_t grid_pol_stride,
                               int grid_size, int num_polarizations, const int16_t *uv,
                               const int16_t *w_plane, const float *weights, void *vis,
                               int64_t num_vis, const void *convolve_kernel, int w_planes,
                               int oversample, int kernel_width, void *workspace,
                               size_t workspace_bytes, int variant, void *stream)
{
    KIMG_CHECK_ARG(grid && uv && w_plane && weights && vis && convolve_kernel);
    KIMG_CHECK_ARG(grid_row_stride >= grid_size);
    int rc = check_f64_args(grid_size, num_polarizations, num_vis, w_planes, oversample,
                            kernel_width, variant);
    if (rc)
        return rc;
    if (num_vis == 0)
        return 0;
    variant &= 0xff;
    hipStream_t s = (hipStream_t) stream;
    if (variant == KIMG_VARIANT_BINNED) {
        kimg_binned_stream b;
        rc = kimg_bin_stream(uv, w_plane, weights, vis, num_vis, grid_size, num_polarizations,
                             w_planes, oversample, kernel_width, workspace, workspace_bytes, s, b);
        if (rc)
            return rc;
        rc = kimg_degrid_window_f64((const double2 *) grid, grid_row_stride, grid_pol_stride,
                                    grid_size, num_polarizations, b.uv, b.w_plane, b.weights, b.vis,
                                    num_vis, (const float2 *) convolve_kernel, w_planes, oversample,
                                    kernel_width, s);
        return rc ? rc : kimg_unbin_vis(b, vis, num_vis, num_polarizations, s);
    }
    if (variant == KIMG_VARIANT_MFMA || (variant == KIMG_VARIANT_AUTO && kernel_width <= WINF))
        return kimg_degrid_window_f64((const double2 *) grid, grid_row_stride, grid_pol_stride,
                                      grid_size, num_polarizations, uv, w_plane, weights,
                                      (float2 *) vis, num_vis, (const float2 *) convolve_kernel,
                                      w_planes, oversample, kernel_width, s);
    int blocks = kimg_divup(num_vis, 4);
    if (blocks > 16384)
        blocks = 16384;
    kimg_for_pols(num_polarizations, [&](auto p) {
        degrid_f64_generic_kernel<decltype(p)::value><<<blocks, 256, 0, s>>>(
            (const double2 *) grid, grid_row_stride, grid_pol_stride, grid_size, uv, w_plane, weights,
            (float2 *) vis, num_vis, (const float2 *) convolve_kernel, w_planes, oversample,
            kernel_width); });
    return kimg_launch_status();
}

// (kimg_preload, api.hip)
KIMG_PRELOAD_THIS_UNIT(grid_f64_generic_kernel<1>)
