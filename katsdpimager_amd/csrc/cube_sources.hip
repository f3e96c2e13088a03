// Source parameters (include/kimg.h, "Source spectra and line parameters"): the label cube of
// cube_link.hip and the cube read once into a ragged table with one entry per (source, channel of its
// box) -- the integrated spectrum of every source -- and that table reduced, a thread per source, to
// flux, error, peak, centroid and the widths at 50 % and 20 % of the peak.  katsdpimager_amd/sources.py
// holds the same contracts as numpy (source_spectra_host, source_lines_host).
//
// The spectra launch has the geometry of cube_link.hip's dense launches (kimg_cube_labels.h): a
// workgroup owns 1024 consecutive elements of ONE channel's plane, a thread four consecutive ones, so
// every element of a wave has the same channel and the destination of a voxel is its label's alone.
// What reaches memory is combined in two steps.  A thread whose four labels are equal adds its four
// values up; a thread whose labels differ flushes the runs of equal labels among its four elements
// itself.  Then the wave reduces over runs of equal labels in LANE order (a segmented reduction: six
// rounds of shuffles, a lane takes its neighbour's partial sum iff no run starts between them), and the
// first lane of every run issues the atomics: a wave whose 256 elements carry one label issues one
// atomic per table, a wave inside a source a few lanes wide one per stretch of it.  A wave without a
// label returns after the label load and reads nothing of the cube.
#include "kimg_cube_labels.h"

namespace {

struct src_shape {
    int64_t M, blocks_per_channel, label_pitch, cube_pitch;
    int label_wide, cube_wide;      // one access for a thread's four labels / four values
};

// The ragged tables.  c0, offsets and total are the caller's: nothing read from them is trusted for
// an address before it has been checked against `total`.
struct src_tables {
    const int32_t *c0, *offsets;
    double *sum;
    int32_t *voxels, *finite;
    int64_t total;
    int N;
};

__device__ inline double src_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

__global__ __launch_bounds__(LK_THREADS)
void src_zero_kernel(double *__restrict__ sum, int32_t *__restrict__ voxels, int32_t *__restrict__ finite,
                     int64_t total)
{
    const int64_t step = (int64_t) gridDim.x * LK_THREADS;
    for (int64_t i = (int64_t) blockIdx.x * LK_THREADS + threadIdx.x; i < total; i += step) {
        sum[i] = 0.0;
        voxels[i] = 0;
        finite[i] = 0;
    }
}

// `voxels` voxels of source `label` (1 .. N) in channel c, `finite` of them finite with sum s
__device__ inline void src_add(const src_tables &t, int32_t label, int c, double s, int voxels, int finite)
{
    const int64_t first = t.c0[label - 1];
    const int64_t from = t.offsets[label - 1], to = t.offsets[label];
    const int64_t at = from + (c - first);
    if (c < first || at >= to || at < 0 || at >= t.total)
        return;
    atomicAdd(t.voxels + at, voxels);
    if (finite) {
        atomicAdd(t.finite + at, finite);
        atomicAdd(t.sum + at, s);
    }
}

__global__ __launch_bounds__(LK_THREADS)
void src_spectra_kernel(const int32_t *__restrict__ labels, const float *__restrict__ cube,
                        const src_shape g, const col_mask filled, const src_tables t)
{
    const int c = (int) (blockIdx.x / g.blocks_per_channel);
    if (!lk_filled(filled, c))
        return;
    const int64_t i = blockIdx.x - c * g.blocks_per_channel;
    const int64_t j = (i * LK_THREADS + threadIdx.x) * LK_V;
    const int n = (int) max((int64_t) 0, min((int64_t) LK_V, g.M - j));
    // (no thread leaves on its own: the shuffles below want the whole wave)
    int32_t l[LK_V] = {0, 0, 0, 0};
    if (n)
        lk_label_load(labels + c * g.label_pitch + j, n, g.label_wide, l);
    bool any = false;
#pragma unroll
    for (int e = 0; e < LK_V; e++) {
        l[e] = l[e] > 0 && l[e] <= t.N ? l[e] : 0;
        any |= l[e] != 0;
    }
    if (!__any(any))
        return;
    float f[LK_V] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (any) {
        const float *from = cube + c * g.cube_pitch + j;
        if (g.cube_wide && n == LK_V) {
            col_load<LK_V>(from, f);
        } else {
#pragma unroll
            for (int e = 0; e < LK_V; e++)
                if (e < n)
                    f[e] = from[e];
        }
    }
    double v[LK_V];
    int ok[LK_V];
#pragma unroll
    for (int e = 0; e < LK_V; e++) {
        ok[e] = (__float_as_uint(f[e]) & 0x7f800000u) != 0x7f800000u;
        v[e] = ok[e] ? (double) f[e] : 0.0;
    }
    // the thread's own part: one label in all four elements goes on to the wave, anything else is
    // flushed here, run by run
    int32_t key = 0;
    double s = 0.0;
    int counts = 0;                 // voxels in bits 0-15, finite ones in bits 16-31
    if (l[0] == l[1] && l[1] == l[2] && l[2] == l[3]) {
        key = l[0];
        s = ((v[0] + v[1]) + v[2]) + v[3];
        counts = LK_V | ((ok[0] + ok[1] + ok[2] + ok[3]) << 16);
    } else {
        int32_t run = 0;
        double run_s = 0.0;
        int run_voxels = 0, run_finite = 0;
#pragma unroll
        for (int e = 0; e < LK_V; e++) {
            if (l[e] != run) {
                if (run)
                    src_add(t, run, c, run_s, run_voxels, run_finite);
                run = l[e];
                run_s = 0.0;
                run_voxels = 0;
                run_finite = 0;
            }
            run_voxels++;
            run_finite += ok[e];
            run_s = run_s + v[e];
        }
        if (run)
            src_add(t, run, c, run_s, run_voxels, run_finite);
    }
    // the wave's: runs of equal keys in lane order.  Before the round with offset `off` a lane holds
    // the sum over itself and the next off - 1 lanes as far as its run goes; it takes the sum of lane
    // + off iff that lane is in its run, that is iff no run starts in (lane, lane + off].
    const int lane = threadIdx.x & (WAVE - 1);
    const int32_t before = __shfl_up(key, 1, WAVE);
    const unsigned long long heads = __ballot(lane == 0 || before != key);
    const unsigned long long above = lane == WAVE - 1 ? 0 : heads >> (lane + 1);
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const double s2 = __shfl_down(s, off, WAVE);
        const int counts2 = __shfl_down(counts, off, WAVE);
        if (lane + off < WAVE && (above & ((1ull << off) - 1)) == 0) {
            s = s + s2;
            counts += counts2;
        }
    }
    if (((heads >> lane) & 1) && key)
        src_add(t, key, c, s, counts & 0xffff, counts >> 16);
}

// ---- lines ------------------------------------------------------------------------------------------

struct src_channels {
    const double *unit, *width, *coord, *variance;      // DEVICE [C] each
    int C;
};

__device__ inline double src_quiet(double x) { return x != x ? src_nan() : x; }

// The spectrum of one source: d(k) = sum[k] * unit[c], x(k) = coord[c], c = first + k
struct src_spectrum {
    const double *sum, *unit, *coord;
    __device__ double d(int k) const { return sum[k] * unit[k]; }
    __device__ double x(int k) const { return coord[k]; }
};

// The two edges at level L (0 < L <= d(peak)): the first k from either end with d(k) >= L, and between
// it and the entry before it the place where the straight line through the two crosses L
__device__ inline void src_edges(const src_spectrum &p, int n, double L, double &lo, double &hi)
{
    int k = 0;
    while (k < n - 1 && !(p.d(k) >= L))
        k++;
    lo = k == 0 ? p.x(0)
                : p.x(k - 1) + (L - p.d(k - 1)) / (p.d(k) - p.d(k - 1)) * (p.x(k) - p.x(k - 1));
    k = n - 1;
    while (k > 0 && !(p.d(k) >= L))
        k--;
    hi = k == n - 1 ? p.x(n - 1)
                    : p.x(k + 1) + (L - p.d(k + 1)) / (p.d(k) - p.d(k + 1)) * (p.x(k) - p.x(k + 1));
}

__global__ __launch_bounds__(LK_THREADS)
void src_lines_kernel(int N, const int32_t *__restrict__ c0, const int32_t *__restrict__ offsets,
                      int64_t total, const double *__restrict__ sum, const int32_t *__restrict__ finite,
                      const src_channels ch, const kimg_source_line_table out)
{
    const int s = blockIdx.x * LK_THREADS + threadIdx.x;
    if (s >= N)
        return;
    const int64_t first = c0[s], from = offsets[s];
    int64_t length = (int64_t) offsets[s + 1] - from;
    // a row that leaves the band or the tables has no entries
    if (first < 0 || from < 0 || length < 0 || first + length > ch.C || from + length > total)
        length = 0;
    const int n = (int) length;
    const src_spectrum p = {sum + from, ch.unit + first, ch.coord + first};
    const double *width = ch.width + first, *variance = ch.variance + first;
    const int32_t *count = finite + from;
    double flux = 0.0, var = 0.0, s0 = 0.0, s1 = 0.0, peak = src_nan();
    int peak_k = -1;
    for (int k = 0; k < n; k++) {
        const double d = p.d(k);
        flux = flux + d * width[k];
        var = var + (double) count[k] * variance[k];
        s0 = s0 + d;
        s1 = s1 + d * p.x(k);
        if (count[k] > 0 && (peak_k < 0 || d > peak)) {
            peak = d;
            peak_k = k;
        }
    }
    double edge[4] = {src_nan(), src_nan(), src_nan(), src_nan()};
    if (peak_k >= 0 && peak > 0.0) {
        src_edges(p, n, 0.5 * peak, edge[0], edge[1]);
        src_edges(p, n, 0.2 * peak, edge[2], edge[3]);
    }
    out.flux[s] = src_quiet(flux);
    out.flux_err[s] = src_quiet(sqrt(var));
    out.peak[s] = src_quiet(peak);
    out.peak_channel[s] = peak_k < 0 ? -1 : (int32_t) (first + peak_k);
    out.centroid[s] = s0 == 0.0 ? src_nan() : src_quiet(s1 / s0);
    out.w50[s] = src_quiet(fabs(edge[1] - edge[0]));
    out.w20[s] = src_quiet(fabs(edge[3] - edge[2]));
    out.w50_lo[s] = src_quiet(edge[0]);
    out.w50_hi[s] = src_quiet(edge[1]);
    out.w20_lo[s] = src_quiet(edge[2]);
    out.w20_hi[s] = src_quiet(edge[3]);
    out.channels[s] = n;
}

bool src_line_table_ok(const kimg_source_line_table *t)
{
    if (!t)
        return false;
    const void *eight[] = {t->flux, t->flux_err, t->peak, t->centroid, t->w50, t->w20, t->w50_lo, t->w50_hi,
                           t->w20_lo, t->w20_hi};
    const void *four[] = {t->peak_channel, t->channels};
    for (const void *p : eight)
        if (!p || !lk_aligned(p, 8))
            return false;
    for (const void *p : four)
        if (!p || !lk_aligned(p, 4))
            return false;
    return true;
}

constexpr int64_t SRC_MAX_TOTAL = (int64_t) INT32_MAX - 1;

}  // namespace

extern "C" int kimg_cube_source_spectra(const int32_t *labels, int64_t label_pitch, const float *cube,
                                        int64_t channel_pitch, int num_channels, int64_t plane_elements,
                                        const uint8_t *filled_host, int num_sources, const int32_t *c0,
                                        const int32_t *offsets, int64_t total, double *sum,
                                        int32_t *voxels, int32_t *finite, void *stream)
{
    const int64_t M = plane_elements;
    KIMG_CHECK_ARG(labels && cube && filled_host && c0 && offsets && sum && voxels && finite);
    KIMG_CHECK_ARG(lk_aligned(labels, 4) && lk_aligned(cube, 4) && lk_aligned(c0, 4) && lk_aligned(offsets, 4)
                   && lk_aligned(voxels, 4) && lk_aligned(finite, 4) && lk_aligned(sum, 8));
    KIMG_CHECK_ARG(num_sources >= 0 && total >= 0);
    KIMG_CHECK_ARG(num_channels >= 1 && M >= 0);
    KIMG_CHECK_ARG(label_pitch >= M && channel_pitch >= M);
    if (!lk_fits(num_channels, M) || total > SRC_MAX_TOTAL)
        return KIMG_EUNSUPPORTED;
    if (num_sources == 0 || M == 0)
        return 0;
    hipStream_t s = (hipStream_t) stream;
    if (total) {
        const unsigned blocks = (unsigned) min((int64_t) 4096, (total + LK_THREADS - 1) / LK_THREADS);
        src_zero_kernel<<<blocks, LK_THREADS, 0, s>>>(sum, voxels, finite, total);
        src_shape g;
        g.M = M;
        g.blocks_per_channel = lk_blocks_per_channel(M);
        g.label_pitch = label_pitch;
        g.cube_pitch = channel_pitch;
        g.label_wide = (((uintptr_t) labels | ((uintptr_t) label_pitch * 4)) & 15) == 0;
        g.cube_wide = (((uintptr_t) cube | ((uintptr_t) channel_pitch * 4)) & 15) == 0;
        const src_tables t = {c0, offsets, sum, voxels, finite, total, num_sources};
        src_spectra_kernel<<<(unsigned) (g.blocks_per_channel * num_channels), LK_THREADS, 0, s>>>(
            labels, cube, g, lk_filled_mask(filled_host, num_channels), t);
    }
    return kimg_launch_status();
}

extern "C" int kimg_source_lines(int num_sources, const int32_t *c0, const int32_t *offsets, int64_t total,
                                 const double *sum, const int32_t *finite, int num_channels,
                                 const double *unit_host, const double *width_host,
                                 const double *coord_host, const double *variance_host,
                                 double *channel_tables, const kimg_source_line_table *lines, void *stream)
{
    KIMG_CHECK_ARG(c0 && offsets && sum && finite && unit_host && width_host && coord_host && variance_host
                   && channel_tables);
    KIMG_CHECK_ARG(lk_aligned(c0, 4) && lk_aligned(offsets, 4) && lk_aligned(finite, 4) && lk_aligned(sum, 8)
                   && lk_aligned(channel_tables, 8));
    KIMG_CHECK_ARG(src_line_table_ok(lines));
    KIMG_CHECK_ARG(num_sources >= 0 && total >= 0);
    KIMG_CHECK_ARG(num_channels >= 1);
    if (num_channels > COL_MAX_CHANNELS || total > SRC_MAX_TOTAL)
        return KIMG_EUNSUPPORTED;
    if (num_sources == 0)
        return 0;
    hipStream_t s = (hipStream_t) stream;
    const int C = num_channels;
    const double *host[4] = {unit_host, width_host, coord_host, variance_host};
    for (int k = 0; k < 4; k++)
        KIMG_HIP(hipMemcpyAsync(channel_tables + (size_t) k * C, host[k], sizeof(double) * C,
                                hipMemcpyHostToDevice, s));
    const src_channels ch = {channel_tables, channel_tables + C, channel_tables + 2 * (size_t) C,
                             channel_tables + 3 * (size_t) C, C};
    src_lines_kernel<<<(unsigned) kimg_divup(num_sources, LK_THREADS), LK_THREADS, 0, s>>>(
        num_sources, c0, offsets, total, sum, finite, ch, *lines);
    return kimg_launch_status();
}

KIMG_PRELOAD_THIS_UNIT(src_zero_kernel)
