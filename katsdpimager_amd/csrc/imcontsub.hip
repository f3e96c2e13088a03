// Image-plane continuum subtraction (include/kimg.h, "Image-plane continuum subtraction"): per element
// of the plane of a cube [C][M], a polynomial of order <= 3 fitted across the line-free channels and
// subtracted from every filled channel, in place or into a second cube; a continuum map, coefficient
// maps, the fit's residual rms and the count of samples come with it.  katsdpimager_amd/imcontsub.py
// holds the same contract as numpy (imcontsub_host).
//
// The column layout is kimg_cube_column.h's (a thread owns V consecutive elements for both channel
// loops, V = 4 with 16-byte loads and stores or 1), the solve kimg_cholesky.h's.  Pass 1 walks the fit
// channels only and keeps the normal equations in registers: K (K + 1) / 2 + K doubles per element,
// 56 doubles per thread at K = 4 and V = 4.  The weights, the basis and the reference values are the
// same for every lane: they come through the scalar path, and so do the products w B_k B_l, which the
// wave forms once per channel.  Pass 2 walks every filled channel: read, subtract, add r * r to R on
// the fit channels, store.  The two masks travel by value; a channel that is out is skipped by a
// uniform branch without a load.  No LDS, no atomics, no scratch.  Traffic per element: 4 bytes per
// fit channel, 8 per filled channel.
#include "kimg_cube_column.h"
#include "kimg_cholesky.h"

namespace {

constexpr int IC_UNROLL = 4;                    // channels whose loads are in flight together
constexpr int IC_MAX_K = KIMG_IMCONTSUB_MAX_ORDER + 1;
constexpr int IC_ALL = KIMG_IMCONTSUB_CONTINUUM | KIMG_IMCONTSUB_COEFFICIENTS | KIMG_IMCONTSUB_RMS
                       | KIMG_IMCONTSUB_COUNT;

struct ic_bref {
    double v[IC_MAX_K];
};

struct ic_out {
    float *continuum, *coefficients, *rms;
    int64_t coefficient_pitch;
    int32_t *count;
};

// The channels a loop visits
struct ic_range {
    int first, stop;
};

// `groups` threads have work: thread t owns the elements t * V .. t * V + V - 1.  `line` may be `cube`
// itself: a thread reads its own elements of a round before it stores any of them.
template <int K, int V>
__global__ __launch_bounds__(COL_THREADS)
void imcontsub_kernel(const float *cube, int64_t pitch, float *line, int64_t line_pitch, int64_t groups,
                      int C, const col_mask filled, const col_mask fit, ic_range fit_range,
                      ic_range filled_range, const double *__restrict__ w,
                      const double *__restrict__ basis, const ic_bref bref, int min_samples, ic_out out)
{
    const int64_t t = (int64_t) blockIdx.x * COL_THREADS + threadIdx.x;
    const bool live = t < groups;
    // (lanes past the plane run along with clamped addresses and store nothing)
    const int64_t j = (live ? t : 0) * V;
    const float *p = cube + j;
    float *q = line + j;

    // A: lower triangle, row by row (A[k (k + 1) / 2 + l], l <= k)
    constexpr int T = K * (K + 1) / 2;
    double A[V][T], b[V][K];
    int n[V];
#pragma unroll
    for (int e = 0; e < V; e++) {
#pragma unroll
        for (int i = 0; i < T; i++)
            A[e][i] = 0.0;
#pragma unroll
        for (int k = 0; k < K; k++)
            b[e][k] = 0.0;
        n[e] = 0;
    }

    for (int c0 = fit_range.first; c0 < fit_range.stop; c0 += IC_UNROLL) {
        float v[IC_UNROLL][V];
        bool on[IC_UNROLL];
        const uint64_t have = col_bits_from(fit, c0);
#pragma unroll
        for (int u = 0; u < IC_UNROLL; u++) {
            const int c = c0 + u;
            on[u] = c < fit_range.stop && ((have >> u) & 1);
#pragma unroll
            for (int e = 0; e < V; e++)
                v[u][e] = col_nan();
            if (on[u])
                col_load<V>(p + (int64_t) c * pitch, v[u]);
        }
#pragma unroll
        for (int u = 0; u < IC_UNROLL; u++) {
            if (!on[u])
                continue;
            const int c = c0 + u;
            // the same for every lane
            const double wc = w[c];
            double wb[K], wbb[T];
#pragma unroll
            for (int k = 0; k < K; k++) {
                wb[k] = wc * basis[(int64_t) k * C + c];
#pragma unroll
                for (int l = 0; l <= k; l++)
                    wbb[k * (k + 1) / 2 + l] = wb[k] * basis[(int64_t) l * C + c];
            }
#pragma unroll
            for (int e = 0; e < V; e++) {
                const bool usable = isfinite(v[u][e]);
                const double I = (double) v[u][e];
                n[e] += usable ? 1 : 0;
#pragma unroll
                for (int k = 0; k < K; k++) {
#pragma unroll
                    for (int l = 0; l <= k; l++) {
                        const int i = k * (k + 1) / 2 + l;
                        A[e][i] = usable ? A[e][i] + wbb[i] : A[e][i];
                    }
                    b[e][k] = usable ? b[e][k] + wb[k] * I : b[e][k];
                }
            }
        }
    }

    const int need = max(K, min_samples);
    double a[V][K];
    bool fitted[V];
#pragma unroll
    for (int e = 0; e < V; e++) {
        fitted[e] = n[e] >= need;
        // (an element that is not fitted solves whatever it has: nothing of it is stored)
        kimg_cholesky<K>(A[e]);
        kimg_cholesky_solve<K>(A[e], b[e], a[e]);
    }

    double R[V];
#pragma unroll
    for (int e = 0; e < V; e++)
        R[e] = 0.0;
    for (int c0 = filled_range.first; c0 < filled_range.stop; c0 += IC_UNROLL) {
        float v[IC_UNROLL][V];
        bool on[IC_UNROLL];
        const uint64_t have = col_bits_from(filled, c0);
        const uint64_t in_fit = col_bits_from(fit, c0);
#pragma unroll
        for (int u = 0; u < IC_UNROLL; u++) {
            const int c = c0 + u;
            on[u] = c < filled_range.stop && ((have >> u) & 1);
#pragma unroll
            for (int e = 0; e < V; e++)
                v[u][e] = col_nan();
            if (on[u])
                col_load<V>(p + (int64_t) c * pitch, v[u]);
        }
#pragma unroll
        for (int u = 0; u < IC_UNROLL; u++) {
            if (!on[u])
                continue;
            const int c = c0 + u;
            const bool fit_channel = (in_fit >> u) & 1;
            double B[K];
#pragma unroll
            for (int k = 0; k < K; k++)
                B[k] = basis[(int64_t) k * C + c];
            float o[V];
#pragma unroll
            for (int e = 0; e < V; e++) {
                double model = 0.0;
#pragma unroll
                for (int k = 0; k < K; k++)
                    model += a[e][k] * B[k];
                const bool usable = isfinite(v[u][e]);
                const double r = (double) v[u][e] - model;
                R[e] = fit_channel && usable ? R[e] + r * r : R[e];
                o[e] = fitted[e] ? (usable ? (float) r : v[u][e]) : col_nan();
            }
            if (live)
                col_store<V>(q + (int64_t) c * line_pitch, o);
        }
    }

    if (!live)
        return;
    float continuum[V], rms[V], coefficient[K][V];
#pragma unroll
    for (int e = 0; e < V; e++) {
        double at_ref = 0.0;
#pragma unroll
        for (int k = 0; k < K; k++) {
            at_ref += a[e][k] * bref.v[k];
            coefficient[k][e] = fitted[e] ? (float) a[e][k] : col_nan();
        }
        continuum[e] = fitted[e] ? (float) at_ref : col_nan();
        const double mean = R[e] / (double) (n[e] - K);
        rms[e] = fitted[e] && n[e] > K ? (float) sqrt(mean) : col_nan();
    }
    if (out.continuum) col_store<V>(out.continuum + j, continuum);
    if (out.coefficients) {
#pragma unroll
        for (int k = 0; k < K; k++)
            col_store<V>(out.coefficients + (int64_t) k * out.coefficient_pitch + j, coefficient[k]);
    }
    if (out.rms) col_store<V>(out.rms + j, rms);
    if (out.count) col_store<V>(out.count + j, n);
}

ic_out ic_offset(const ic_out &o, int64_t by)
{
    ic_out r = o;
    if (r.continuum) r.continuum += by;
    if (r.coefficients) r.coefficients += by;
    if (r.rms) r.rms += by;
    if (r.count) r.count += by;
    return r;
}

// [first, stop): from the first to the last channel of the mask
ic_range ic_range_of(const col_mask &mask, int C)
{
    ic_range r = {0, 0};
    bool any = false;
    for (int c = 0; c < C; c++)
        if ((mask.bits[c >> 5] >> (c & 31)) & 1u) {
            if (!any)
                r.first = c;
            any = true;
            r.stop = c + 1;
        }
    return r;
}

}  // namespace

extern "C" int kimg_imcontsub(const float *cube, int64_t channel_pitch, float *line,
                              int64_t line_channel_pitch, int num_channels, int64_t plane_elements,
                              const uint8_t *filled_host, const uint8_t *fit_host,
                              const double *w_host, const double *w, const double *basis, int order,
                              double bref0, double bref1, double bref2, double bref3,
                              int min_samples, int outputs, float *continuum, float *coefficients,
                              int64_t coefficient_pitch, float *rms, int32_t *count, void *stream)
{
    KIMG_CHECK_ARG(order >= 0 && order <= KIMG_IMCONTSUB_MAX_ORDER && num_channels >= 1);
    KIMG_CHECK_ARG(filled_host && fit_host && w_host);
    const int K = order + 1;
    if (num_channels > COL_MAX_CHANNELS)
        return KIMG_EUNSUPPORTED;
    // a channel enters the fit iff it is asked for, filled and weighted: one mask
    col_mask filled = {}, fit = {};
    int fit_channels = 0;
    for (int c = 0; c < num_channels; c++) {
        if (!filled_host[c])
            continue;
        col_set(filled, c);
        if (fit_host[c] && w_host[c] > 0.0 && w_host[c] < INFINITY) {
            col_set(fit, c);
            fit_channels++;
        }
    }
    if (fit_channels < K || !col_plane_fits(plane_elements))
        return KIMG_EUNSUPPORTED;
    KIMG_CHECK_ARG(cube && line && w && basis && plane_elements >= 0);
    KIMG_CHECK_ARG(min_samples >= 1 && min_samples <= num_channels);
    KIMG_CHECK_ARG(channel_pitch >= plane_elements && line_channel_pitch >= plane_elements);
    KIMG_CHECK_ARG(outputs != 0 && (outputs & ~IC_ALL) == 0);
    KIMG_CHECK_ARG(((uintptr_t) cube & 3) == 0 && ((uintptr_t) line & 3) == 0);
    KIMG_CHECK_ARG(((uintptr_t) w & 7) == 0 && ((uintptr_t) basis & 7) == 0);
    ic_out out;
    out.continuum = (outputs & KIMG_IMCONTSUB_CONTINUUM) ? continuum : nullptr;
    out.coefficients = (outputs & KIMG_IMCONTSUB_COEFFICIENTS) ? coefficients : nullptr;
    out.rms = (outputs & KIMG_IMCONTSUB_RMS) ? rms : nullptr;
    out.count = (outputs & KIMG_IMCONTSUB_COUNT) ? count : nullptr;
    out.coefficient_pitch = coefficient_pitch;
    const void *ptrs[4] = {out.continuum, out.coefficients, out.rms, out.count};
    const int bits[4] = {KIMG_IMCONTSUB_CONTINUUM, KIMG_IMCONTSUB_COEFFICIENTS, KIMG_IMCONTSUB_RMS,
                         KIMG_IMCONTSUB_COUNT};
    uintptr_t alignment = (uintptr_t) cube | ((uintptr_t) channel_pitch * sizeof(float))
                          | (uintptr_t) line | ((uintptr_t) line_channel_pitch * sizeof(float));
    for (int i = 0; i < 4; i++) {
        if (outputs & bits[i]) {
            KIMG_CHECK_ARG(ptrs[i] && ((uintptr_t) ptrs[i] & 3) == 0);
            alignment |= (uintptr_t) ptrs[i];
        }
    }
    if (out.coefficients) {
        KIMG_CHECK_ARG(coefficient_pitch >= plane_elements);
        alignment |= (uintptr_t) coefficient_pitch * sizeof(float);
    }
    // in place (the same cube, the same pitch), or two cubes that share no byte
    if (!(line == cube && line_channel_pitch == channel_pitch)) {
        const uintptr_t from = (uintptr_t) cube, to = (uintptr_t) line;
        const uintptr_t from_bytes =
            ((uintptr_t) (num_channels - 1) * channel_pitch + plane_elements) * sizeof(float);
        const uintptr_t to_bytes =
            ((uintptr_t) (num_channels - 1) * line_channel_pitch + plane_elements) * sizeof(float);
        KIMG_CHECK_ARG(from + from_bytes <= to || to + to_bytes <= from);
    }
    if (plane_elements == 0)
        return 0;

    const ic_bref bref = {{bref0, bref1, bref2, bref3}};
    const ic_range fit_range = ic_range_of(fit, num_channels);
    const ic_range filled_range = ic_range_of(filled, num_channels);
    hipStream_t s = (hipStream_t) stream;
    auto launch = [&](auto v, const float *from, float *to, int64_t groups, const ic_out &maps) {
        constexpr int V = decltype(v)::value;
        kimg_for_pols(K, [&](auto k) {      // (K is 1 .. 4, like a polarization count)
            imcontsub_kernel<decltype(k)::value, V><<<col_blocks(groups), COL_THREADS, 0, s>>>(
                from, channel_pitch, to, line_channel_pitch, groups, num_channels, filled, fit,
                fit_range, filled_range, w, basis, bref, min_samples, maps);
        });
    };
    const int64_t done = col_vector_elements(alignment, plane_elements);
    if (done)
        launch(std::integral_constant<int, 4>{}, cube, line, done / 4, out);
    if (done < plane_elements)
        launch(std::integral_constant<int, 1>{}, cube + done, line + done, plane_elements - done,
               ic_offset(out, done));
    return kimg_launch_status();
}

KIMG_PRELOAD_THIS_UNIT((imcontsub_kernel<1, 1>))
