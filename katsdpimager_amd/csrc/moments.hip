// Moment maps (include/kimg.h, "Moment maps"): a cube [C][M] of images reduced along its channel axis
// to integrated intensity, intensity-weighted coordinate, dispersion, peak and coordinate of the peak
// over the samples above a per-channel cut.  katsdpimager_amd/cube.py holds the same contract as numpy
// (moments_host), and the order of every sum below is that contract's: the device has the twin's bits.
//
// One kernel, a column reduction: a thread owns V consecutive elements of the plane (V = 4 with
// 16-byte loads, or 1) for the whole channel loop, so no sum crosses threads and the order of
// summation is the loop's.  Adjacent lanes take adjacent elements: a wave reads 1 KiB (V = 4) or 256 B
// of one channel per load.  The channel loop is unrolled by MM_UNROLL with all loads of a round issued
// before the first is consumed; a thread has 64 bytes in flight at V = 4.  The per-channel tables are
// uniform across the wave: x and cut come through scalar loads, `filled` as a bit mask by value in the
// kernel arguments, and a channel that is not filled is skipped by a uniform branch without a load.
// With select_hanning the three-channel window lives in registers (prev, cur and the round's loads of
// the NEXT channels), so every voxel is still read once.  A NaN stands for "no neighbour" in that
// window -- outside the range, not filled or not finite are one case under the replicate rule.
#include "kimg_cube_column.h"
#include "kimg_moment_math.h"

namespace {

constexpr int MM_THREADS = COL_THREADS;
constexpr int MM_UNROLL = 4;                    // channels whose loads are in flight together
constexpr int MM_MAX_CHANNELS = KIMG_MOMENTS_MAX_CHANNELS;
constexpr int MM_ALL = KIMG_MOMENT_0 | KIMG_MOMENT_1 | KIMG_MOMENT_2 | KIMG_MOMENT_8 | KIMG_MOMENT_9
                       | KIMG_MOMENT_COUNT;

struct mm_out {
    float *m0, *m1, *m2, *m8, *m9;
    int32_t *count;
};

// `groups` threads have work: thread t owns the elements t * V .. t * V + V - 1
template <int V, bool HANNING, bool SECOND>
__global__ __launch_bounds__(MM_THREADS)
void moments_kernel(const float *__restrict__ cube, int64_t pitch, int64_t groups, int first, int stop,
                    const double *__restrict__ x, const float *__restrict__ cut,
                    const col_mask filled, double width, mm_out out)
{
    const int64_t t = (int64_t) blockIdx.x * MM_THREADS + threadIdx.x;
    const bool live = t < groups;
    // (lanes past the plane run along with clamped addresses and store nothing)
    const int64_t j = (live ? t : 0) * V;
    const float *p = cube + j;
    const double x_ref = x[(first + stop) / 2];
    mm_acc acc[V];
#pragma unroll
    for (int e = 0; e < V; e++) {
        acc[e].S0 = acc[e].S1 = acc[e].S2 = 0.0;
        acc[e].peak = -INFINITY;
        acc[e].n = 0;
        acc[e].pc = first;
    }

    if constexpr (!HANNING) {
        for (int c0 = first; c0 < stop; c0 += MM_UNROLL) {
            float v[MM_UNROLL][V];
            bool on[MM_UNROLL];
            const uint64_t have = col_bits_from(filled, c0);
#pragma unroll
            for (int u = 0; u < MM_UNROLL; u++) {
                const int c = c0 + u;
                on[u] = c < stop && ((have >> u) & 1);
#pragma unroll
                for (int e = 0; e < V; e++)
                    v[u][e] = col_nan();
                if (on[u])
                    col_load<V>(p + (int64_t) c * pitch, v[u]);
            }
#pragma unroll
            for (int u = 0; u < MM_UNROLL; u++) {
                if (on[u]) {
                    const int c = c0 + u;
                    const double d = x[c] - x_ref;
                    const double ct = (double) cut[c];
#pragma unroll
                    for (int e = 0; e < V; e++)
                        mm_add<SECOND>(acc[e], v[u][e], (double) v[u][e], ct, d, c);
                }
            }
        }
    } else {
        float prev[V], cur[V];
#pragma unroll
        for (int e = 0; e < V; e++)
            prev[e] = cur[e] = col_nan();
        if (col_bits_from(filled, first) & 1)
            col_load<V>(p + (int64_t) first * pitch, cur);
        for (int c0 = first; c0 < stop; c0 += MM_UNROLL) {
            float next[MM_UNROLL][V];       // the channels c0 + 1 .. c0 + MM_UNROLL
            const uint64_t have = col_bits_from(filled, c0);
#pragma unroll
            for (int u = 0; u < MM_UNROLL; u++) {
                const int c = c0 + u + 1;
#pragma unroll
                for (int e = 0; e < V; e++)
                    next[u][e] = col_nan();
                if (c < stop && ((have >> (u + 1)) & 1))
                    col_load<V>(p + (int64_t) c * pitch, next[u]);
            }
#pragma unroll
            for (int u = 0; u < MM_UNROLL; u++) {
                const int c = c0 + u;
                if (c < stop) {
                    const double d = x[c] - x_ref;
                    const double ct = (double) cut[c];
#pragma unroll
                    for (int e = 0; e < V; e++) {
                        const float I = cur[e];
                        const float a = isfinite(prev[e]) ? prev[e] : I;
                        const float b = isfinite(next[u][e]) ? next[u][e] : I;
                        const double s = ((0.25 * (double) a) + (0.5 * (double) I)) + (0.25 * (double) b);
                        mm_add<SECOND>(acc[e], I, s, ct, d, c);
                        prev[e] = I;
                        cur[e] = next[u][e];
                    }
                }
            }
        }
    }

    if (!live)
        return;
    float m0[V], m1[V], m2[V], m8[V], m9[V];
    int32_t n[V];
#pragma unroll
    for (int e = 0; e < V; e++) {
        const mm_values v = mm_finish<SECOND>(acc[e], width, x_ref);
        n[e] = acc[e].n;
        m0[e] = v.m0;
        m1[e] = v.m1;
        m2[e] = v.m2;
        m8[e] = v.m8;
        m9[e] = col_nan();
        if (out.m9 && v.any)
            m9[e] = (float) x[acc[e].pc];
    }
    if (out.m0) col_store<V>(out.m0 + j, m0);
    if (out.m1) col_store<V>(out.m1 + j, m1);
    if (out.m2) col_store<V>(out.m2 + j, m2);
    if (out.m8) col_store<V>(out.m8 + j, m8);
    if (out.m9) col_store<V>(out.m9 + j, m9);
    if (out.count) col_store<V>(out.count + j, n);
}

template <int V>
void mm_launch(const float *cube, int64_t pitch, int64_t groups, int first, int stop, const double *x,
               const float *cut, const col_mask &filled, double width, bool hanning, bool second,
               const mm_out &out, hipStream_t s)
{
    const unsigned blocks = col_blocks(groups);
    auto go = [&](auto h, auto m) {
        moments_kernel<V, decltype(h)::value, decltype(m)::value><<<blocks, MM_THREADS, 0, s>>>(
            cube, pitch, groups, first, stop, x, cut, filled, width, out);
    };
    using yes = std::true_type;
    using no = std::false_type;
    if (hanning)
        second ? go(yes{}, yes{}) : go(yes{}, no{});
    else
        second ? go(no{}, yes{}) : go(no{}, no{});
}

mm_out mm_offset(const mm_out &o, int64_t by)
{
    mm_out r = o;
    if (r.m0) r.m0 += by;
    if (r.m1) r.m1 += by;
    if (r.m2) r.m2 += by;
    if (r.m8) r.m8 += by;
    if (r.m9) r.m9 += by;
    if (r.count) r.count += by;
    return r;
}

}  // namespace

extern "C" int kimg_moments(const float *cube, int64_t channel_pitch, int num_channels,
                            int64_t plane_elements, int first, int stop, const double *x,
                            const float *cut, const uint8_t *filled_host, double width,
                            int select_hanning, int outputs, float *moment0, float *moment1,
                            float *moment2, float *moment8, float *moment9, int32_t *count,
                            void *stream)
{
    KIMG_CHECK_ARG(cube && x && cut && filled_host);
    KIMG_CHECK_ARG(num_channels >= 1 && plane_elements >= 0);
    KIMG_CHECK_ARG(first >= 0 && first < stop && stop <= num_channels);
    KIMG_CHECK_ARG(channel_pitch >= plane_elements);
    KIMG_CHECK_ARG(width == width);
    KIMG_CHECK_ARG(outputs != 0 && (outputs & ~MM_ALL) == 0);
    mm_out out;
    out.m0 = (outputs & KIMG_MOMENT_0) ? moment0 : nullptr;
    out.m1 = (outputs & KIMG_MOMENT_1) ? moment1 : nullptr;
    out.m2 = (outputs & KIMG_MOMENT_2) ? moment2 : nullptr;
    out.m8 = (outputs & KIMG_MOMENT_8) ? moment8 : nullptr;
    out.m9 = (outputs & KIMG_MOMENT_9) ? moment9 : nullptr;
    out.count = (outputs & KIMG_MOMENT_COUNT) ? count : nullptr;
    const void *ptrs[6] = {out.m0, out.m1, out.m2, out.m8, out.m9, out.count};
    const int bits[6] = {KIMG_MOMENT_0, KIMG_MOMENT_1, KIMG_MOMENT_2, KIMG_MOMENT_8, KIMG_MOMENT_9,
                         KIMG_MOMENT_COUNT};
    uintptr_t alignment = (uintptr_t) cube | ((uintptr_t) channel_pitch * sizeof(float));
    for (int i = 0; i < 6; i++) {
        if (outputs & bits[i]) {
            KIMG_CHECK_ARG(ptrs[i] && ((uintptr_t) ptrs[i] & 3) == 0);
            alignment |= (uintptr_t) ptrs[i];
        }
    }
    KIMG_CHECK_ARG(((uintptr_t) cube & 3) == 0 && ((uintptr_t) x & 7) == 0 && ((uintptr_t) cut & 3) == 0);
    if (num_channels > MM_MAX_CHANNELS || !col_plane_fits(plane_elements))
        return KIMG_EUNSUPPORTED;
    if (plane_elements == 0)
        return 0;

    col_mask filled = {};
    for (int c = 0; c < num_channels; c++)
        if (filled_host[c])
            col_set(filled, c);
    const bool second = outputs & (KIMG_MOMENT_1 | KIMG_MOMENT_2);
    const bool hanning = select_hanning != 0;
    hipStream_t s = (hipStream_t) stream;
    // the form (kimg_cube_column.h): four elements per thread where every address a thread forms is
    // 16-byte aligned, one element per thread for the tail and for everything else
    const int64_t done = col_vector_elements(alignment, plane_elements);
    if (done)
        mm_launch<4>(cube, channel_pitch, done / 4, first, stop, x, cut, filled, width, hanning, second,
                     out, s);
    if (done < plane_elements)
        mm_launch<1>(cube + done, channel_pitch, plane_elements - done, first, stop, x, cut, filled,
                     width, hanning, second, mm_offset(out, done), s);
    return kimg_launch_status();
}

KIMG_PRELOAD_THIS_UNIT((moments_kernel<1, false, false>))
