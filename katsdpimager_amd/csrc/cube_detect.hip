// Detection mask (include/kimg.h, "Detection mask"): the pieces of a smooth-and-clip source finder on
// a cube [C][M] that the library did not have -- a spectral boxcar with replacement of what is blank
// or already detected, the restoring of blanks after a spatial smoothing, the threshold against
// kimg_cube_stats' sigma table OR-ed into a byte mask [C][M], the pruning of runs of detected channels
// that are too short, and the mask applied to a cube for kimg_moments.  katsdpimager_amd/detect.py
// holds the same contracts as numpy (boxcar_host, reblank_host, threshold_host, prune_host,
// apply_host) and the finder that strings them together with kimg_cube_smooth and kimg_cube_stats.
//
// The column layout is kimg_cube_column.h's: a thread owns V consecutive elements of the plane (V = 4
// with 16-byte float accesses, or 1) for a whole channel loop, nothing crosses threads.  The mask of
// those four elements is one 4-byte access where the mask's base and pitch are 4-byte aligned (MV) and
// four byte accesses where not; what a kernel sets or clears in the mask it stores byte by byte, under
// the lane's own condition, so that no byte is written that the contract does not name.
//
// The boxcar's window.  The sum is a direct one -- w terms in ascending channel order for every output,
// no running window -- so a voxel is needed by up to w outputs of its own thread.  It is kept in LDS:
// a workgroup is ONE wave, a ring of `slots` rows [slot][64 * V] holds the last channels, and a lane
// reads back only what it wrote itself (its V consecutive words of a row: one ds_read_b128 at V = 4,
// conflict-free as in spectrum_stats.hip), so there is no barrier.  A round stages BX_UNROLL channels
// -- their loads issued together -- and then writes BX_UNROLL outputs; every cube voxel comes from
// memory once whatever the width.  The ring holds w + 2 * BX_UNROLL - 2 channels at most, rounded up
// to a power of two: 8 rows at w = 1, 16 up to w = 7, 32 at w = 15, 64 (64 KiB at V = 4) at w = 31.
// The ring keeps a value as it was read, with +0 in place of a finite value that the mask removes:
// what is not finite is told apart when it is read back (it counts as +0 in the sum and, with
// `blank`, makes the output of its own channel NaN).
#include "kimg_cube_column.h"

namespace {

constexpr int DT_UNROLL = 4;                    // channels whose loads are in flight together
constexpr int BX_THREADS = WAVE;                // the boxcar's workgroup: one wave
constexpr int BX_UNROLL = 4;

__device__ inline bool dt_finite(float x)
{
    return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u;
}

// The mask bytes of V consecutive elements
template <int V, bool MV> __device__ inline void dt_mask_load(const uint8_t *p, uint8_t (&b)[V])
{
    if constexpr (V == 4 && MV) {
        const uint32_t t = *reinterpret_cast<const uint32_t *>(p);
        b[0] = (uint8_t) t; b[1] = (uint8_t) (t >> 8); b[2] = (uint8_t) (t >> 16); b[3] = (uint8_t) (t >> 24);
    } else {
#pragma unroll
        for (int e = 0; e < V; e++)
            b[e] = p[e];
    }
}

// The rounds of a column walk: for every DT_UNROLL channels from 0, load(u, c) for each filled channel
// c = c0 + u of the round -- all of them issued first -- then use(u, c) for the same channels
template <class L, class U>
__device__ inline void dt_walk(int num_channels, const col_mask &filled, L &&load, U &&use)
{
    for (int c0 = 0; c0 < num_channels; c0 += DT_UNROLL) {
        const uint64_t have = col_bits_from(filled, c0);
        if (!(have & ((1u << DT_UNROLL) - 1)))
            continue;
        bool on[DT_UNROLL];
#pragma unroll
        for (int u = 0; u < DT_UNROLL; u++) {
            on[u] = c0 + u < num_channels && ((have >> u) & 1);
            if (on[u])
                load(u, c0 + u);
        }
#pragma unroll
        for (int u = 0; u < DT_UNROLL; u++)
            if (on[u])
                use(u, c0 + u);
    }
}

// ---- boxcar -----------------------------------------------------------------------------------------

template <int V> __device__ inline void bx_row(const float *row, float (&v)[V])
{
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4 *>(row);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = *row;
    }
}

template <int V> __device__ inline void bx_set_row(float *row, const float (&v)[V])
{
    if constexpr (V == 4)
        *reinterpret_cast<float4 *>(row) = make_float4(v[0], v[1], v[2], v[3]);
    else
        *row = v[0];
}

// `groups` threads have work: thread t owns the elements t * V .. t * V + V - 1.  slots: a power of
// two, at least 2 * h + 2 * BX_UNROLL - 1
template <int V, bool MV>
__global__ __launch_bounds__(BX_THREADS)
void dt_boxcar_kernel(const float *__restrict__ cube, int64_t pitch, const uint8_t *__restrict__ mask,
                      int64_t mask_pitch, float *__restrict__ out, int64_t out_pitch, int64_t groups,
                      int num_channels, const col_mask filled, int h, int slots, int blank)
{
    extern __shared__ __align__(16) float bx_ring[];        // [slots][BX_THREADS * V]
    constexpr int ROW = BX_THREADS * V;
    const int64_t t = (int64_t) blockIdx.x * BX_THREADS + threadIdx.x;
    const bool live = t < groups;
    // (lanes past the plane run along with clamped addresses and store nothing)
    const int64_t j = (live ? t : 0) * V;
    float *mine = bx_ring + V * threadIdx.x;
    const int wrap = slots - 1;
    const double w = (double) (2 * h + 1);

    int staged = 0;         // channels below this are in the ring (or have left it)
    for (int c0 = 0; c0 < num_channels; c0 += BX_UNROLL) {
        // what the outputs of this round read: the channels below c0 + BX_UNROLL + h
        const int need = min(c0 + BX_UNROLL + h, num_channels);
        for (; staged < need; staged += BX_UNROLL) {
            const uint64_t have = col_bits_from(filled, staged);
            float v[BX_UNROLL][V];
            uint8_t b[BX_UNROLL][V];
#pragma unroll
            for (int u = 0; u < BX_UNROLL; u++) {
                const int c = staged + u;
#pragma unroll
                for (int e = 0; e < V; e++) {
                    v[u][e] = 0.0f;
                    b[u][e] = 0;
                }
                if (c < num_channels && ((have >> u) & 1)) {
                    col_load<V>(cube + j + (int64_t) c * pitch, v[u]);
                    if (mask)
                        dt_mask_load<V, MV>(mask + j + (int64_t) c * mask_pitch, b[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < BX_UNROLL; u++) {
                const int c = staged + u;
                if (c < num_channels) {
#pragma unroll
                    for (int e = 0; e < V; e++)
                        v[u][e] = (b[u][e] && dt_finite(v[u][e])) ? 0.0f : v[u][e];
                    bx_set_row<V>(mine + (c & wrap) * ROW, v[u]);
                }
            }
        }
        const uint64_t have = col_bits_from(filled, c0);
#pragma unroll 1
        for (int u = 0; u < BX_UNROLL; u++) {
            const int c = c0 + u;
            if (c >= num_channels || !((have >> u) & 1))
                continue;
            // (channels outside the band are +0.0 terms: they leave acc, which is never -0.0, as it is)
            const int lo = max(c - h, 0), hi = min(c + h, num_channels - 1);
            double acc[V];
#pragma unroll
            for (int e = 0; e < V; e++)
                acc[e] = 0.0;
#pragma unroll 4
            for (int k = lo; k <= hi; k++) {
                float z[V];
                bx_row<V>(mine + (k & wrap) * ROW, z);
#pragma unroll
                for (int e = 0; e < V; e++)
                    acc[e] = acc[e] + (double) (dt_finite(z[e]) ? z[e] : 0.0f);
            }
            float own[V], r[V];
            bx_row<V>(mine + (c & wrap) * ROW, own);
#pragma unroll
            for (int e = 0; e < V; e++) {
                r[e] = (float) (acc[e] / w);
                r[e] = (blank && !dt_finite(own[e])) ? col_nan() : r[e];
            }
            if (live)
                col_store<V>(out + j + (int64_t) c * out_pitch, r);
        }
    }
}

// ---- reblank ----------------------------------------------------------------------------------------

template <int V>
__global__ __launch_bounds__(COL_THREADS)
void dt_reblank_kernel(float *__restrict__ work, int64_t work_pitch, const float *__restrict__ cube,
                       int64_t pitch, int64_t groups, int num_channels, const col_mask filled)
{
    const int64_t t = (int64_t) blockIdx.x * COL_THREADS + threadIdx.x;
    const bool live = t < groups;
    const int64_t j = (live ? t : 0) * V;
    float v[DT_UNROLL][V];
    dt_walk(num_channels, filled,
        [&](int u, int c) { col_load<V>(cube + j + (int64_t) c * pitch, v[u]); },
        [&](int u, int c) {
            float *to = work + j + (int64_t) c * work_pitch;
#pragma unroll
            for (int e = 0; e < V; e++)
                if (live && !dt_finite(v[u][e]))
                    to[e] = col_nan();
        });
}

// ---- threshold --------------------------------------------------------------------------------------

// plane: H * W, the elements of a polarization; origin: the element of the plane that this launch's
// element 0 is (the polarization of an element comes from there); groups_per_channel: 1 or P
template <int V, int POLARITY>
__global__ __launch_bounds__(COL_THREADS)
void dt_threshold_kernel(const float *__restrict__ work, int64_t work_pitch, uint8_t *__restrict__ mask,
                         int64_t mask_pitch, int64_t groups, int num_channels, const col_mask filled,
                         int64_t plane, int64_t origin, const float *__restrict__ sigma,
                         int groups_per_channel, float threshold)
{
    const int64_t t = (int64_t) blockIdx.x * COL_THREADS + threadIdx.x;
    const bool live = t < groups;
    const int64_t j = (live ? t : 0) * V;
    int g[V];
#pragma unroll
    for (int e = 0; e < V; e++)
        g[e] = groups_per_channel == 1 ? 0 : (int) ((origin + j + e) / plane);
    float v[DT_UNROLL][V];
    dt_walk(num_channels, filled,
        [&](int u, int c) { col_load<V>(work + j + (int64_t) c * work_pitch, v[u]); },
        [&](int u, int c) {
            uint8_t *to = mask + j + (int64_t) c * mask_pitch;
            const float *row = sigma + (int64_t) c * groups_per_channel;
#pragma unroll
            for (int e = 0; e < V; e++) {
                const float cut = threshold * row[g[e]];
                const float s = v[u][e];
                bool over;
                if constexpr (POLARITY == KIMG_DETECT_POSITIVE)
                    over = s > cut;
                else if constexpr (POLARITY == KIMG_DETECT_NEGATIVE)
                    over = -s > cut;
                else
                    over = fabsf(s) > cut;
                if (live && dt_finite(s) && over)
                    to[e] = 1;
            }
        });
}

// ---- prune ------------------------------------------------------------------------------------------

// Every channel of the mask is walked.  Per element: `len`, the length of the run of set bytes that
// ends at the previous channel, and `odd`, whether a byte of that run is not 1 while the run is still
// below min_channels.  A run that ends short is cleared behind the walk, one that reaches
// min_channels with an odd byte is written as 1 behind it: both loops are rare and only touch bytes
// of this thread that the walk has already passed.
template <int V, bool MV>
__global__ __launch_bounds__(COL_THREADS)
void dt_prune_kernel(uint8_t *mask, int64_t mask_pitch, int64_t groups, int num_channels,
                     int min_channels)
{
    const int64_t t = (int64_t) blockIdx.x * COL_THREADS + threadIdx.x;
    const bool live = t < groups;
    const int64_t j = (live ? t : 0) * V;
    uint8_t *p = mask + j;
    int len[V];
    bool odd[V];
#pragma unroll
    for (int e = 0; e < V; e++) {
        len[e] = 0;
        odd[e] = false;
    }
    for (int c0 = 0; c0 < num_channels; c0 += DT_UNROLL) {
        uint8_t b[DT_UNROLL][V];
#pragma unroll
        for (int u = 0; u < DT_UNROLL; u++) {
#pragma unroll
            for (int e = 0; e < V; e++)
                b[u][e] = 0;
            if (c0 + u < num_channels)
                dt_mask_load<V, MV>(p + (int64_t) (c0 + u) * mask_pitch, b[u]);
        }
#pragma unroll
        for (int u = 0; u < DT_UNROLL; u++) {
            const int c = c0 + u;
            if (c >= num_channels)
                break;
#pragma unroll
            for (int e = 0; e < V; e++) {
                if (!live)
                    continue;
                if (b[u][e]) {
                    len[e]++;
                    if (len[e] < min_channels) {
                        odd[e] = odd[e] || b[u][e] != 1;
                    } else {
                        if (b[u][e] != 1)
                            p[e + (int64_t) c * mask_pitch] = 1;
                        if (len[e] == min_channels && odd[e])
                            for (int k = c - len[e] + 1; k < c; k++)
                                p[e + (int64_t) k * mask_pitch] = 1;
                        odd[e] = false;
                    }
                } else {
                    if (len[e] > 0 && len[e] < min_channels)
                        for (int k = c - len[e]; k < c; k++)
                            p[e + (int64_t) k * mask_pitch] = 0;
                    len[e] = 0;
                    odd[e] = false;
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < V; e++)
        if (live && len[e] > 0 && len[e] < min_channels)
            for (int k = num_channels - len[e]; k < num_channels; k++)
                p[e + (int64_t) k * mask_pitch] = 0;
}

// ---- apply ------------------------------------------------------------------------------------------

// (`line` may be the cube itself: no __restrict__ on the two)
template <int V, bool MV>
__global__ __launch_bounds__(COL_THREADS)
void dt_apply_kernel(const float *cube, int64_t pitch, const uint8_t *__restrict__ mask,
                     int64_t mask_pitch, float *line, int64_t line_pitch, int64_t groups,
                     int num_channels, const col_mask filled, int invert)
{
    const int64_t t = (int64_t) blockIdx.x * COL_THREADS + threadIdx.x;
    const bool live = t < groups;
    const int64_t j = (live ? t : 0) * V;
    float v[DT_UNROLL][V];
    uint8_t b[DT_UNROLL][V];
    dt_walk(num_channels, filled,
        [&](int u, int c) {
            col_load<V>(cube + j + (int64_t) c * pitch, v[u]);
            dt_mask_load<V, MV>(mask + j + (int64_t) c * mask_pitch, b[u]);
        },
        [&](int u, int c) {
            float r[V];
#pragma unroll
            for (int e = 0; e < V; e++)
                r[e] = ((b[u][e] != 0) != (invert != 0)) ? v[u][e] : col_nan();
            if (live)
                col_store<V>(line + j + (int64_t) c * line_pitch, r);
        });
}

// ---- host -------------------------------------------------------------------------------------------

// The C planes of a cube of `bytes`-sized elements, as a range of addresses
struct dt_extent {
    uintptr_t from, bytes;
};

dt_extent dt_extent_of(const void *p, int64_t pitch, int num_channels, int64_t plane_elements,
                       size_t element)
{
    return {(uintptr_t) p, ((uintptr_t) (num_channels - 1) * pitch + plane_elements) * element};
}

bool dt_disjoint(const dt_extent &a, const dt_extent &b)
{
    return a.from + a.bytes <= b.from || b.from + b.bytes <= a.from;
}

col_mask dt_filled(const uint8_t *filled_host, int num_channels)
{
    col_mask filled = {};
    for (int c = 0; c < num_channels; c++)
        if (filled_host[c])
            col_set(filled, c);
    return filled;
}

// What every entry checks of a cube [C][M]: the counts, and then (after its own KIMG_EINVALs) the limits
bool dt_counts_ok(int num_channels, int64_t plane_elements)
{
    return num_channels >= 1 && plane_elements >= 0;
}

bool dt_float_ok(const void *p, int64_t pitch, int64_t plane_elements)
{
    return p && ((uintptr_t) p & 3) == 0 && pitch >= plane_elements;
}

uintptr_t dt_float_alignment(const void *p, int64_t pitch)
{
    return (uintptr_t) p | ((uintptr_t) pitch * sizeof(float));
}

// The mask's four bytes of a thread are one access iff its base and pitch are 4-byte aligned
bool dt_mask_vector(const void *mask, int64_t mask_pitch)
{
    return (((uintptr_t) mask | (uintptr_t) mask_pitch) & 3) == 0;
}

int bx_slots(int h)
{
    int slots = 8;
    while (slots < 2 * h + 2 * BX_UNROLL - 1)
        slots *= 2;
    return slots;
}

template <int V, bool MV>
int bx_launch(const float *cube, int64_t pitch, const uint8_t *mask, int64_t mask_pitch, float *out,
              int64_t out_pitch, int64_t from, int64_t groups, int num_channels, const col_mask &filled,
              int h, int blank, hipStream_t s)
{
    const int slots = bx_slots(h);
    const size_t lds = (size_t) slots * BX_THREADS * V * sizeof(float);
    if (lds >= 64 * 1024)
        if (const int rc = kimg_dynamic_lds(reinterpret_cast<const void *>(&dt_boxcar_kernel<V, MV>), lds))
            return rc;
    const unsigned blocks = (unsigned) kimg_divup(groups, BX_THREADS);
    dt_boxcar_kernel<V, MV><<<blocks, BX_THREADS, lds, s>>>(
        cube + from, pitch, mask ? mask + from : nullptr, mask_pitch, out + from, out_pitch, groups,
        num_channels, filled, h, slots, blank);
    return 0;
}

}  // namespace

extern "C" int kimg_cube_boxcar(const float *cube, int64_t channel_pitch, const uint8_t *mask,
                                int64_t mask_pitch, float *out, int64_t out_channel_pitch,
                                int num_channels, int64_t plane_elements, const uint8_t *filled_host,
                                int width, int blank, void *stream)
{
    KIMG_CHECK_ARG(cube && out && filled_host);
    KIMG_CHECK_ARG(dt_counts_ok(num_channels, plane_elements));
    KIMG_CHECK_ARG(dt_float_ok(cube, channel_pitch, plane_elements));
    KIMG_CHECK_ARG(dt_float_ok(out, out_channel_pitch, plane_elements));
    KIMG_CHECK_ARG(!mask || mask_pitch >= plane_elements);
    KIMG_CHECK_ARG(width >= 1 && width <= KIMG_BOXCAR_MAX_WIDTH && (width & 1) == 1);
    if (num_channels > COL_MAX_CHANNELS || plane_elements > (int64_t) 0x7fffffff * BX_THREADS)
        return KIMG_EUNSUPPORTED;
    KIMG_CHECK_ARG(dt_disjoint(dt_extent_of(cube, channel_pitch, num_channels, plane_elements, 4),
                               dt_extent_of(out, out_channel_pitch, num_channels, plane_elements, 4)));
    if (plane_elements == 0)
        return 0;
    const col_mask filled = dt_filled(filled_host, num_channels);
    const int h = width / 2;
    hipStream_t s = (hipStream_t) stream;
    const uintptr_t alignment = dt_float_alignment(cube, channel_pitch)
                                | dt_float_alignment(out, out_channel_pitch);
    const bool mv = !mask || dt_mask_vector(mask, mask_pitch);
    const int64_t done = col_vector_elements(alignment, plane_elements);
    if (done) {
        const int rc = mv ? bx_launch<4, true>(cube, channel_pitch, mask, mask_pitch, out,
                                               out_channel_pitch, 0, done / 4, num_channels, filled, h,
                                               blank, s)
                          : bx_launch<4, false>(cube, channel_pitch, mask, mask_pitch, out,
                                                out_channel_pitch, 0, done / 4, num_channels, filled, h,
                                                blank, s);
        if (rc)
            return rc;
    }
    if (done < plane_elements)
        if (const int rc = bx_launch<1, false>(cube, channel_pitch, mask, mask_pitch, out,
                                               out_channel_pitch, done, plane_elements - done,
                                               num_channels, filled, h, blank, s))
            return rc;
    return kimg_launch_status();
}

extern "C" int kimg_cube_reblank(float *work, int64_t work_channel_pitch, const float *cube,
                                 int64_t channel_pitch, int num_channels, int64_t plane_elements,
                                 const uint8_t *filled_host, void *stream)
{
    KIMG_CHECK_ARG(work && cube && filled_host);
    KIMG_CHECK_ARG(dt_counts_ok(num_channels, plane_elements));
    KIMG_CHECK_ARG(dt_float_ok(work, work_channel_pitch, plane_elements));
    KIMG_CHECK_ARG(dt_float_ok(cube, channel_pitch, plane_elements));
    if (num_channels > COL_MAX_CHANNELS || !col_plane_fits(plane_elements))
        return KIMG_EUNSUPPORTED;
    KIMG_CHECK_ARG(dt_disjoint(dt_extent_of(cube, channel_pitch, num_channels, plane_elements, 4),
                               dt_extent_of(work, work_channel_pitch, num_channels, plane_elements, 4)));
    if (plane_elements == 0)
        return 0;
    const col_mask filled = dt_filled(filled_host, num_channels);
    hipStream_t s = (hipStream_t) stream;
    // (the stores are single floats: only the cube's loads have a 16-byte form)
    const int64_t done = col_vector_elements(dt_float_alignment(cube, channel_pitch), plane_elements);
    if (done)
        dt_reblank_kernel<4><<<col_blocks(done / 4), COL_THREADS, 0, s>>>(
            work, work_channel_pitch, cube, channel_pitch, done / 4, num_channels, filled);
    if (done < plane_elements)
        dt_reblank_kernel<1><<<col_blocks(plane_elements - done), COL_THREADS, 0, s>>>(
            work + done, work_channel_pitch, cube + done, channel_pitch, plane_elements - done,
            num_channels, filled);
    return kimg_launch_status();
}

namespace {

template <int V>
void dt_threshold_launch(const float *work, int64_t work_pitch, uint8_t *mask, int64_t mask_pitch,
                         int64_t from, int64_t groups, int num_channels, const col_mask &filled,
                         int64_t plane, const float *sigma, int groups_per_channel, float threshold,
                         int polarity, hipStream_t s)
{
    auto go = [&](auto p) {
        dt_threshold_kernel<V, decltype(p)::value><<<col_blocks(groups), COL_THREADS, 0, s>>>(
            work, work_pitch, mask, mask_pitch, groups, num_channels, filled, plane, from, sigma,
            groups_per_channel, threshold);
    };
    switch (polarity) {
    case KIMG_DETECT_POSITIVE: go(std::integral_constant<int, KIMG_DETECT_POSITIVE>{}); break;
    case KIMG_DETECT_NEGATIVE: go(std::integral_constant<int, KIMG_DETECT_NEGATIVE>{}); break;
    default: go(std::integral_constant<int, KIMG_DETECT_BOTH>{}); break;
    }
}

}  // namespace

extern "C" int kimg_cube_threshold(const float *work, int64_t work_channel_pitch, uint8_t *mask,
                                   int64_t mask_pitch, int num_channels, int num_polarizations,
                                   int height, int width, const uint8_t *filled_host,
                                   const float *sigma, int groups, float threshold, int polarity,
                                   void *stream)
{
    KIMG_CHECK_ARG(work && mask && filled_host && sigma);
    KIMG_CHECK_ARG(num_channels >= 1 && num_polarizations >= 1 && height >= 1 && width >= 1);
    const int64_t plane = (int64_t) height * width;
    KIMG_CHECK_ARG(plane <= INT64_MAX / 4 / num_polarizations);
    const int64_t plane_elements = plane * num_polarizations;
    KIMG_CHECK_ARG(dt_float_ok(work, work_channel_pitch, plane_elements));
    KIMG_CHECK_ARG(mask_pitch >= plane_elements && ((uintptr_t) sigma & 3) == 0);
    KIMG_CHECK_ARG(groups == 1 || groups == num_polarizations);
    KIMG_CHECK_ARG(threshold > 0.0f && threshold < INFINITY);      // (false for NaN)
    KIMG_CHECK_ARG(polarity == KIMG_DETECT_POSITIVE || polarity == KIMG_DETECT_NEGATIVE
                   || polarity == KIMG_DETECT_BOTH);
    if (num_channels > COL_MAX_CHANNELS || !col_plane_fits(plane_elements))
        return KIMG_EUNSUPPORTED;
    const col_mask filled = dt_filled(filled_host, num_channels);
    hipStream_t s = (hipStream_t) stream;
    // (the mask is stored byte by byte: only the work cube's loads have a 16-byte form)
    const int64_t done = col_vector_elements(dt_float_alignment(work, work_channel_pitch), plane_elements);
    if (done)
        dt_threshold_launch<4>(work, work_channel_pitch, mask, mask_pitch, 0, done / 4, num_channels,
                               filled, plane, sigma, groups, threshold, polarity, s);
    if (done < plane_elements)
        dt_threshold_launch<1>(work + done, work_channel_pitch, mask + done, mask_pitch, done,
                               plane_elements - done, num_channels, filled, plane, sigma, groups,
                               threshold, polarity, s);
    return kimg_launch_status();
}

extern "C" int kimg_cube_mask_prune(uint8_t *mask, int64_t mask_pitch, int num_channels,
                                    int64_t plane_elements, int min_channels, void *stream)
{
    KIMG_CHECK_ARG(mask);
    KIMG_CHECK_ARG(dt_counts_ok(num_channels, plane_elements));
    KIMG_CHECK_ARG(mask_pitch >= plane_elements);
    KIMG_CHECK_ARG(min_channels >= 1 && min_channels <= num_channels);
    if (num_channels > COL_MAX_CHANNELS || !col_plane_fits(plane_elements))
        return KIMG_EUNSUPPORTED;
    if (plane_elements == 0)
        return 0;
    hipStream_t s = (hipStream_t) stream;
    const int64_t done = dt_mask_vector(mask, mask_pitch) ? plane_elements & ~(int64_t) 3 : 0;
    if (done)
        dt_prune_kernel<4, true><<<col_blocks(done / 4), COL_THREADS, 0, s>>>(
            mask, mask_pitch, done / 4, num_channels, min_channels);
    if (done < plane_elements)
        dt_prune_kernel<1, false><<<col_blocks(plane_elements - done), COL_THREADS, 0, s>>>(
            mask + done, mask_pitch, plane_elements - done, num_channels, min_channels);
    return kimg_launch_status();
}

extern "C" int kimg_cube_mask_apply(const float *cube, int64_t channel_pitch, const uint8_t *mask,
                                    int64_t mask_pitch, float *line, int64_t line_channel_pitch,
                                    int num_channels, int64_t plane_elements,
                                    const uint8_t *filled_host, int invert, void *stream)
{
    KIMG_CHECK_ARG(cube && mask && line && filled_host);
    KIMG_CHECK_ARG(dt_counts_ok(num_channels, plane_elements));
    KIMG_CHECK_ARG(dt_float_ok(cube, channel_pitch, plane_elements));
    KIMG_CHECK_ARG(dt_float_ok(line, line_channel_pitch, plane_elements));
    KIMG_CHECK_ARG(mask_pitch >= plane_elements);
    if (num_channels > COL_MAX_CHANNELS || !col_plane_fits(plane_elements))
        return KIMG_EUNSUPPORTED;
    // in place (the same cube, the same pitch), or two cubes that share no byte
    if (!(line == cube && line_channel_pitch == channel_pitch))
        KIMG_CHECK_ARG(dt_disjoint(dt_extent_of(cube, channel_pitch, num_channels, plane_elements, 4),
                                   dt_extent_of(line, line_channel_pitch, num_channels, plane_elements, 4)));
    if (plane_elements == 0)
        return 0;
    const col_mask filled = dt_filled(filled_host, num_channels);
    hipStream_t s = (hipStream_t) stream;
    const uintptr_t alignment = dt_float_alignment(cube, channel_pitch)
                                | dt_float_alignment(line, line_channel_pitch);
    const int64_t done = col_vector_elements(alignment, plane_elements);
    if (done) {
        if (dt_mask_vector(mask, mask_pitch))
            dt_apply_kernel<4, true><<<col_blocks(done / 4), COL_THREADS, 0, s>>>(
                cube, channel_pitch, mask, mask_pitch, line, line_channel_pitch, done / 4,
                num_channels, filled, invert);
        else
            dt_apply_kernel<4, false><<<col_blocks(done / 4), COL_THREADS, 0, s>>>(
                cube, channel_pitch, mask, mask_pitch, line, line_channel_pitch, done / 4,
                num_channels, filled, invert);
    }
    if (done < plane_elements)
        dt_apply_kernel<1, false><<<col_blocks(plane_elements - done), COL_THREADS, 0, s>>>(
            cube + done, channel_pitch, mask + done, mask_pitch, line + done, line_channel_pitch,
            plane_elements - done, num_channels, filled, invert);
    return kimg_launch_status();
}

KIMG_PRELOAD_THIS_UNIT((dt_apply_kernel<1, false>))
