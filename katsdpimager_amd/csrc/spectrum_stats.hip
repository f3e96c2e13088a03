// Spectrum statistics (include/kimg.h, "Spectrum statistics"): for every element of the plane of a
// cube [C][M] the count of finite samples along the channel axis, their min, max and median and a
// robust sigma, by exact selection, and optionally the cube with that median subtracted from every
// filled channel.  katsdpimager_amd/spectrum_stats.py holds the same contract as numpy
// (spectrum_stats_host).
//
// The column layout is kimg_cube_column.h's: a thread owns V consecutive elements of the plane (V = 4
// with 16-byte loads and stores, or 1) for a whole channel loop, nothing crosses threads.  What is new
// against moments.hip is that every element wants a rank of its own (n differs per element), so the
// selection is made of steps whose CONTROL is the same for every lane while the ranks are not.
//
// Keys are cube_stats.hip's: key(x) = bits ^ (sign ? 0xffffffff : 0x80000000) for the values, 0x80000000 |
// abs bits for |x| and |x - m|.  The finite values have keys 0x00800000 .. 0xff7fffff and the absolute
// ones 0x80000000 .. 0xff800000, so 0xffffffff (SS_NONE) is no sample's key in either order.
//
// Two forms.
//
// RESIDENT (S entering channels up to SS_RESIDENT_LIMIT): a workgroup is ONE wave; it reads its
// elements' entering channels once and keeps their keys in LDS, [channel][element], a row of 64 * V
// words.  A lane reads back only what it wrote -- its V consecutive words of every row, one
// ds_read_b128 at V = 4, which the LDS serves in groups of 8 lanes x 16 bytes = 32 consecutive banks,
// conflict-free; one word a lane at V = 1, 64 consecutive banks -- so there is no barrier in the
// kernel.  The rank is found by bisection on the key, bit by bit from the top: 32 walks over the S
// rows that count the keys below prefix | bit.  One more walk gives the second middle rank (the count
// of keys <= lo and the smallest key above lo).  For sigma one walk rewrites the rows in place as the
// keys of |x - m| or |x| and the same bisection runs again.  The cube is read once for all five maps.
// The tile: LDS per workgroup is S * 256 * V bytes, so at V = 4 a CU's 160 KiB hold 160 / S
// workgroups of one wave: 2 at S = 64 .. 80, 4 at S = 40.  SS_RESIDENT_LIMIT = 80 is the largest S that
// still has two workgroups a CU (one stages while the other selects); a tile of more than one wave
// would only lower that.  Above 64 KiB the kernel's dynamic-LDS attribute is raised
// (kimg_dynamic_lds).
//
// STREAMING (any S): a radix select on 4-bit digits from the top down, 16 counters per element in
// registers (64 at V = 4, indexed by unrolled constants only), the column re-read from memory in each
// of the 8 passes; one more pass for the second middle rank.  9 reads of the entering channels for
// the median, 9 more for sigma under either estimator.
//
// Channels that do not enter are skipped by a uniform branch without a load, as in moments.hip.
// The line pass is a plain column pass over all filled channels after the maps exist.
#include "kimg_cube_column.h"

namespace {

constexpr int SS_TILE_THREADS = WAVE;           // the resident form's workgroup: one wave
constexpr int SS_RESIDENT_LIMIT = 80;
// AUTO: resident up to here.  Measured: 3 x faster than streaming at S = 16, level with
// it at S = 64 and 80, where two workgroups of one wave a CU leave the LDS reads unhidden
constexpr int SS_AUTO_RESIDENT = 63;
constexpr int SS_UNROLL = 4;                    // channels whose loads are in flight together
constexpr int SS_ALL = KIMG_SPECTRUM_MEDIAN | KIMG_SPECTRUM_SIGMA | KIMG_SPECTRUM_MIN
                       | KIMG_SPECTRUM_MAX | KIMG_SPECTRUM_COUNT;
constexpr uint32_t SS_NONE = 0xffffffffu;       // in place of the key of what is not a sample

// which key a select orders by
constexpr int SS_BY_VALUE = 0;                  // key(x)
constexpr int SS_BY_ABS = 1;                    // key(|x|)
constexpr int SS_BY_DEVIATION = 2;              // key(|x - m|)

struct ss_out {
    float *median, *sigma, *vmin, *vmax;
    int32_t *count;
};

__device__ inline uint32_t ss_key(uint32_t bits)
{
    return bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u);
}

__device__ inline float ss_value(uint32_t key)
{
    return __uint_as_float((key & 0x80000000u) ? key ^ 0x80000000u : ~key);
}

__device__ inline bool ss_finite(uint32_t bits) { return (bits & 0x7f800000u) != 0x7f800000u; }

// The key of a finite x in the order of MODE (m: the element's median)
template <int MODE> __device__ inline uint32_t ss_key_of(float x, float m)
{
    if constexpr (MODE == SS_BY_VALUE)
        return ss_key(__float_as_uint(x));
    else if constexpr (MODE == SS_BY_ABS)
        return 0x80000000u | __float_as_uint(x);
    else
        return 0x80000000u | __float_as_uint(x - m);
}

__device__ inline float ss_middle(uint32_t lo, uint32_t hi) { return (ss_value(lo) + ss_value(hi)) / 2.0f; }

// f(c, v) for every channel c of first .. stop - 1 that is in `mask`, v its V values of this thread:
// the loads of a round are issued before the first is consumed
template <int V, class F>
__device__ inline void ss_walk(const float *p, int64_t pitch, int first, int stop, const col_mask &mask,
                               F &&f)
{
    for (int c0 = first; c0 < stop; c0 += SS_UNROLL) {
        const uint64_t have = col_bits_from(mask, c0);
        if (!(have & ((1u << SS_UNROLL) - 1)))
            continue;
        float v[SS_UNROLL][V];
        bool on[SS_UNROLL];
#pragma unroll
        for (int u = 0; u < SS_UNROLL; u++) {
            const int c = c0 + u;
            on[u] = c < stop && ((have >> u) & 1);
#pragma unroll
            for (int e = 0; e < V; e++)
                v[u][e] = 0.0f;
            if (on[u])
                col_load<V>(p + (int64_t) c * pitch, v[u]);
        }
#pragma unroll
        for (int u = 0; u < SS_UNROLL; u++)
            if (on[u])
                f(c0 + u, v[u]);
    }
}

// What both forms end with: the maps of this thread's V elements.  lo, hi: the keys of the two
// middle ranks by value; slo, shi: by |x| or |x - m|
template <int V>
__device__ inline void ss_store(const ss_out &out, int64_t j, int min_samples, const uint32_t (&n)[V],
                                const uint32_t (&kmin)[V], const uint32_t (&kmax)[V],
                                const float (&m)[V], const uint32_t (&slo)[V], const uint32_t (&shi)[V])
{
    float median[V], sigma[V], vmin[V], vmax[V];
    int32_t count[V];
#pragma unroll
    for (int e = 0; e < V; e++) {
        const bool enough = n[e] >= (uint32_t) min_samples;
        count[e] = (int32_t) n[e];
        median[e] = enough ? m[e] : col_nan();
        vmin[e] = enough ? ss_value(kmin[e]) : col_nan();
        vmax[e] = enough ? ss_value(kmax[e]) : col_nan();
        sigma[e] = enough ? ss_middle(slo[e], shi[e]) * KIMG_CUBE_STATS_TO_RMS : col_nan();
    }
    if (out.median) col_store<V>(out.median + j, median);
    if (out.sigma) col_store<V>(out.sigma + j, sigma);
    if (out.vmin) col_store<V>(out.vmin + j, vmin);
    if (out.vmax) col_store<V>(out.vmax + j, vmax);
    if (out.count) col_store<V>(out.count + j, count);
}

// ---- resident ---------------------------------------------------------------------------------------

template <int V> __device__ inline void ss_row(const uint32_t *row, uint32_t (&k)[V])
{
    if constexpr (V == 4) {
        const uint4 t = *reinterpret_cast<const uint4 *>(row);
        k[0] = t.x; k[1] = t.y; k[2] = t.z; k[3] = t.w;
    } else {
        k[0] = *row;
    }
}

template <int V> __device__ inline void ss_set_row(uint32_t *row, const uint32_t (&k)[V])
{
    if constexpr (V == 4)
        *reinterpret_cast<uint4 *>(row) = make_uint4(k[0], k[1], k[2], k[3]);
    else
        *row = k[0];
}

// The keys of ranks k0 and k1 (k0 <= k1 <= k0 + 1) among this thread's S rows: lo by bisection -- the
// largest t with #(keys < t) <= k0 --, hi from the count of keys <= lo and the smallest key above
template <int V>
__device__ inline void ss_resident_select(const uint32_t *mine, int S, const uint32_t (&k0)[V],
                                          const uint32_t (&k1)[V], uint32_t (&lo)[V], uint32_t (&hi)[V])
{
    constexpr int ROW = SS_TILE_THREADS * V;
#pragma unroll
    for (int e = 0; e < V; e++)
        lo[e] = 0;
    for (int b = 31; b >= 0; b--) {
        uint32_t candidate[V], below[V];
#pragma unroll
        for (int e = 0; e < V; e++) {
            candidate[e] = lo[e] | (1u << b);
            below[e] = 0;
        }
#pragma unroll 4
        for (int s = 0; s < S; s++) {
            uint32_t k[V];
            ss_row<V>(mine + s * ROW, k);
#pragma unroll
            for (int e = 0; e < V; e++)
                below[e] += k[e] < candidate[e] ? 1u : 0u;
        }
#pragma unroll
        for (int e = 0; e < V; e++)
            lo[e] = below[e] <= k0[e] ? candidate[e] : lo[e];
    }
    uint32_t upto[V], next[V];
#pragma unroll
    for (int e = 0; e < V; e++) {
        upto[e] = 0;
        next[e] = SS_NONE;
    }
#pragma unroll 4
    for (int s = 0; s < S; s++) {
        uint32_t k[V];
        ss_row<V>(mine + s * ROW, k);
#pragma unroll
        for (int e = 0; e < V; e++) {
            upto[e] += k[e] <= lo[e] ? 1u : 0u;
            next[e] = k[e] > lo[e] ? min(next[e], k[e]) : next[e];
        }
    }
#pragma unroll
    for (int e = 0; e < V; e++)
        hi[e] = upto[e] > k1[e] ? lo[e] : next[e];
}

// `groups` threads have work: thread t owns the elements t * V .. t * V + V - 1
template <int V>
__global__ __launch_bounds__(SS_TILE_THREADS)
void ss_resident_kernel(const float *__restrict__ cube, int64_t pitch, int64_t groups, int first,
                        int stop, const col_mask enter, int S, int estimator, int min_samples,
                        ss_out out)
{
    extern __shared__ __align__(16) uint32_t ss_rows[];     // [S][SS_TILE_THREADS * V]
    constexpr int ROW = SS_TILE_THREADS * V;
    const int64_t t = (int64_t) blockIdx.x * SS_TILE_THREADS + threadIdx.x;
    const bool live = t < groups;
    // (lanes past the plane run along with clamped addresses and store nothing)
    const int64_t j = (live ? t : 0) * V;
    uint32_t *mine = ss_rows + V * threadIdx.x;

    // the entering channels, once: keys into the rows, with n, min and max on the way
    uint32_t n[V], kmin[V], kmax[V];
#pragma unroll
    for (int e = 0; e < V; e++) {
        n[e] = 0;
        kmin[e] = SS_NONE;
        kmax[e] = 0;
    }
    int slot = 0;
    ss_walk<V>(cube + j, pitch, first, stop, enter, [&](int, const float (&v)[V]) {
        uint32_t k[V];
#pragma unroll
        for (int e = 0; e < V; e++) {
            const uint32_t bits = __float_as_uint(v[e]);
            const bool ok = ss_finite(bits);
            k[e] = ok ? ss_key(bits) : SS_NONE;
            n[e] += ok ? 1u : 0u;
            kmin[e] = min(kmin[e], k[e]);
            kmax[e] = ok ? max(kmax[e], k[e]) : kmax[e];
        }
        ss_set_row<V>(mine + slot * ROW, k);
        slot++;
    });

    uint32_t k0[V], k1[V], lo[V], hi[V], slo[V], shi[V];
    float m[V];
#pragma unroll
    for (int e = 0; e < V; e++) {
        k0[e] = n[e] ? (n[e] - 1) / 2 : 0;
        k1[e] = n[e] / 2;
        slo[e] = shi[e] = 0x80000000u;
    }
    ss_resident_select<V>(mine, S, k0, k1, lo, hi);
#pragma unroll
    for (int e = 0; e < V; e++)
        m[e] = ss_middle(lo[e], hi[e]);
    if (out.sigma) {
        // the rows once more, in place: the keys of |x - m| or |x|
        const bool deviation = estimator == KIMG_CUBE_STATS_MAD;
        for (int s = 0; s < S; s++) {
            uint32_t k[V];
            ss_row<V>(mine + s * ROW, k);
#pragma unroll
            for (int e = 0; e < V; e++) {
                const float x = ss_value(k[e]);
                const uint32_t now = deviation ? ss_key_of<SS_BY_DEVIATION>(x, m[e])
                                               : ss_key_of<SS_BY_ABS>(x, m[e]);
                k[e] = k[e] == SS_NONE ? SS_NONE : now;
            }
            ss_set_row<V>(mine + s * ROW, k);
        }
        ss_resident_select<V>(mine, S, k0, k1, slo, shi);
    }
    if (live)
        ss_store<V>(out, j, min_samples, n, kmin, kmax, m, slo, shi);
}

// ---- streaming --------------------------------------------------------------------------------------

// One pass over the column: counts of the 4-bit digit at `shift` among the samples whose key agrees
// with `prefix` above it.  TOP: the first pass (every sample counts; min and max by value)
template <int V, int MODE, bool TOP>
__device__ inline void ss_stream_pass(const float *p, int64_t pitch, int first, int stop,
                                      const col_mask &enter, const float (&m)[V], int shift,
                                      const uint32_t (&prefix)[V], uint32_t (&counts)[V][16],
                                      uint32_t (&kmin)[V], uint32_t (&kmax)[V])
{
#pragma unroll
    for (int e = 0; e < V; e++)
#pragma unroll
        for (int d = 0; d < 16; d++)
            counts[e][d] = 0;
    ss_walk<V>(p, pitch, first, stop, enter, [&](int, const float (&v)[V]) {
#pragma unroll
        for (int e = 0; e < V; e++) {
            const bool ok = ss_finite(__float_as_uint(v[e]));
            const uint32_t key = ss_key_of<MODE>(v[e], m[e]);
            bool in = ok;
            if constexpr (!TOP)
                in = ok && (key >> (shift + 4)) == prefix[e];
            // (16: no digit)
            const uint32_t digit = in ? (key >> shift) & 15u : 16u;
#pragma unroll
            for (int d = 0; d < 16; d++)
                counts[e][d] += digit == (uint32_t) d ? 1u : 0u;
            if constexpr (TOP && MODE == SS_BY_VALUE) {
                kmin[e] = ok ? min(kmin[e], key) : kmin[e];
                kmax[e] = ok ? max(kmax[e], key) : kmax[e];
            }
        }
    });
}

// The digit whose bin holds rank k, appended to the prefix; k becomes the rank inside the bin
template <int V>
__device__ inline void ss_descend(const uint32_t (&counts)[V][16], uint32_t (&prefix)[V], uint32_t (&k)[V])
{
#pragma unroll
    for (int e = 0; e < V; e++) {
        uint32_t digit = 0, left = k[e];
        bool found = false;
#pragma unroll
        for (int d = 0; d < 16; d++) {
            const bool here = !found && left < counts[e][d];
            digit = here ? (uint32_t) d : digit;
            found = found || here;
            left = found ? left : left - counts[e][d];
        }
        prefix[e] = (prefix[e] << 4) | digit;
        k[e] = left;
    }
}

// The keys of the two middle ranks in the order of MODE.  SS_BY_VALUE makes n, min and max on the way;
// the other orders take n as it is (the samples are the same)
template <int V, int MODE>
__device__ inline void ss_stream_select(const float *p, int64_t pitch, int first, int stop,
                                        const col_mask &enter, const float (&m)[V], uint32_t (&n)[V],
                                        uint32_t (&kmin)[V], uint32_t (&kmax)[V], uint32_t (&lo)[V],
                                        uint32_t (&hi)[V])
{
    uint32_t counts[V][16], k[V];
#pragma unroll
    for (int e = 0; e < V; e++)
        lo[e] = 0;
    ss_stream_pass<V, MODE, true>(p, pitch, first, stop, enter, m, 28, lo, counts, kmin, kmax);
#pragma unroll
    for (int e = 0; e < V; e++) {
        if constexpr (MODE == SS_BY_VALUE) {
            uint32_t total = 0;
#pragma unroll
            for (int d = 0; d < 16; d++)
                total += counts[e][d];
            n[e] = total;
        }
        k[e] = n[e] ? (n[e] - 1) / 2 : 0;
    }
    ss_descend<V>(counts, lo, k);
    for (int shift = 24; shift >= 0; shift -= 4) {
        ss_stream_pass<V, MODE, false>(p, pitch, first, stop, enter, m, shift, lo, counts, kmin, kmax);
        ss_descend<V>(counts, lo, k);
    }
    // the second middle rank: the count of keys <= lo and the smallest key above lo
    uint32_t upto[V], next[V];
#pragma unroll
    for (int e = 0; e < V; e++) {
        upto[e] = 0;
        next[e] = SS_NONE;
    }
    ss_walk<V>(p, pitch, first, stop, enter, [&](int, const float (&v)[V]) {
#pragma unroll
        for (int e = 0; e < V; e++) {
            const bool ok = ss_finite(__float_as_uint(v[e]));
            const uint32_t key = ss_key_of<MODE>(v[e], m[e]);
            upto[e] += ok && key <= lo[e] ? 1u : 0u;
            next[e] = ok && key > lo[e] ? min(next[e], key) : next[e];
        }
    });
#pragma unroll
    for (int e = 0; e < V; e++)
        hi[e] = upto[e] > n[e] / 2 ? lo[e] : next[e];
}

template <int V>
__global__ __launch_bounds__(COL_THREADS)
void ss_streaming_kernel(const float *__restrict__ cube, int64_t pitch, int64_t groups, int first,
                         int stop, const col_mask enter, int estimator, int min_samples, ss_out out)
{
    const int64_t t = (int64_t) blockIdx.x * COL_THREADS + threadIdx.x;
    const bool live = t < groups;
    const int64_t j = (live ? t : 0) * V;
    const float *p = cube + j;
    uint32_t n[V], kmin[V], kmax[V], lo[V], hi[V], slo[V], shi[V];
    float m[V];
#pragma unroll
    for (int e = 0; e < V; e++) {
        n[e] = 0;
        kmin[e] = SS_NONE;
        kmax[e] = 0;
        m[e] = 0.0f;
        slo[e] = shi[e] = 0x80000000u;
    }
    ss_stream_select<V, SS_BY_VALUE>(p, pitch, first, stop, enter, m, n, kmin, kmax, lo, hi);
#pragma unroll
    for (int e = 0; e < V; e++)
        m[e] = ss_middle(lo[e], hi[e]);
    if (out.sigma) {
        if (estimator == KIMG_CUBE_STATS_MAD)
            ss_stream_select<V, SS_BY_DEVIATION>(p, pitch, first, stop, enter, m, n, kmin, kmax, slo, shi);
        else
            ss_stream_select<V, SS_BY_ABS>(p, pitch, first, stop, enter, m, n, kmin, kmax, slo, shi);
    }
    if (live)
        ss_store<V>(out, j, min_samples, n, kmin, kmax, m, slo, shi);
}

// ---- the line pass ----------------------------------------------------------------------------------

// line[c][m] = cube[c][m] - median[m] for every filled channel; the median map holds NaN exactly where
// n < min_samples (the median of finite samples is never NaN).  `line` may be the cube itself.
template <int V>
__global__ __launch_bounds__(COL_THREADS)
void ss_line_kernel(const float *cube, int64_t pitch, float *line, int64_t line_pitch, int64_t groups,
                    int num_channels, const col_mask filled, const float *__restrict__ median)
{
    const int64_t t = (int64_t) blockIdx.x * COL_THREADS + threadIdx.x;
    const bool live = t < groups;
    const int64_t j = (live ? t : 0) * V;
    float m[V];
    col_load<V>(median + j, m);
    float *to = line + j;
    ss_walk<V>(cube + j, pitch, 0, num_channels, filled, [&](int c, const float (&v)[V]) {
        float r[V];
#pragma unroll
        for (int e = 0; e < V; e++)
            r[e] = m[e] != m[e] ? col_nan() : v[e] - m[e];
        if (live)
            col_store<V>(to + (int64_t) c * line_pitch, r);
    });
}

ss_out ss_offset(const ss_out &o, int64_t by)
{
    ss_out r = o;
    if (r.median) r.median += by;
    if (r.sigma) r.sigma += by;
    if (r.vmin) r.vmin += by;
    if (r.vmax) r.vmax += by;
    if (r.count) r.count += by;
    return r;
}

// One thread per group of V elements in workgroups of one wave: the plane the resident launch covers
inline bool ss_plane_fits(int64_t plane_elements)
{
    return plane_elements <= (int64_t) 0x7fffffff * SS_TILE_THREADS;
}

struct ss_call {
    const float *cube;
    int64_t pitch;
    int first, stop, S;
    col_mask enter;
    int estimator, min_samples;
    bool resident;
    hipStream_t stream;
};

template <int V> int ss_launch(const ss_call &a, int64_t from, int64_t groups, const ss_out &out)
{
    if (a.resident) {
        const size_t lds = (size_t) a.S * SS_TILE_THREADS * V * sizeof(uint32_t);
        if (lds > 64 * 1024)
            if (const int rc = kimg_dynamic_lds(reinterpret_cast<const void *>(&ss_resident_kernel<V>), lds))
                return rc;
        const unsigned blocks = (unsigned) kimg_divup(groups, SS_TILE_THREADS);
        ss_resident_kernel<V><<<blocks, SS_TILE_THREADS, lds, a.stream>>>(
            a.cube + from, a.pitch, groups, a.first, a.stop, a.enter, a.S, a.estimator, a.min_samples, out);
    } else {
        ss_streaming_kernel<V><<<col_blocks(groups), COL_THREADS, 0, a.stream>>>(
            a.cube + from, a.pitch, groups, a.first, a.stop, a.enter, a.estimator, a.min_samples, out);
    }
    return 0;
}

}  // namespace

extern "C" int kimg_spectrum_stats_resident_limit(void) { return SS_RESIDENT_LIMIT; }

extern "C" int kimg_spectrum_stats(const float *cube, int64_t channel_pitch, int num_channels,
                                   int64_t plane_elements, int first, int stop,
                                   const uint8_t *stat_host, const uint8_t *filled_host, int estimator,
                                   int min_samples, int outputs, float *median, float *sigma,
                                   float *min, float *max, int32_t *count, float *line,
                                   int64_t line_channel_pitch, int form, void *stream)
{
    KIMG_CHECK_ARG(cube && stat_host && filled_host);
    KIMG_CHECK_ARG(num_channels >= 1 && plane_elements >= 0);
    KIMG_CHECK_ARG(first >= 0 && first < stop && stop <= num_channels);
    KIMG_CHECK_ARG(channel_pitch >= plane_elements);
    KIMG_CHECK_ARG(estimator == KIMG_CUBE_STATS_MEDIAN_ABS || estimator == KIMG_CUBE_STATS_MAD);
    KIMG_CHECK_ARG(min_samples >= 1);
    KIMG_CHECK_ARG(outputs != 0 && (outputs & ~SS_ALL) == 0);
    KIMG_CHECK_ARG(form == KIMG_SPECTRUM_FORM_AUTO || form == KIMG_SPECTRUM_FORM_RESIDENT
                   || form == KIMG_SPECTRUM_FORM_STREAMING);
    KIMG_CHECK_ARG(((uintptr_t) cube & 3) == 0);
    ss_out out;
    out.median = (outputs & KIMG_SPECTRUM_MEDIAN) ? median : nullptr;
    out.sigma = (outputs & KIMG_SPECTRUM_SIGMA) ? sigma : nullptr;
    out.vmin = (outputs & KIMG_SPECTRUM_MIN) ? min : nullptr;
    out.vmax = (outputs & KIMG_SPECTRUM_MAX) ? max : nullptr;
    out.count = (outputs & KIMG_SPECTRUM_COUNT) ? count : nullptr;
    const void *ptrs[5] = {out.median, out.sigma, out.vmin, out.vmax, out.count};
    const int bits[5] = {KIMG_SPECTRUM_MEDIAN, KIMG_SPECTRUM_SIGMA, KIMG_SPECTRUM_MIN, KIMG_SPECTRUM_MAX,
                         KIMG_SPECTRUM_COUNT};
    uintptr_t alignment = (uintptr_t) cube | ((uintptr_t) channel_pitch * sizeof(float));
    for (int i = 0; i < 5; i++) {
        if (outputs & bits[i]) {
            KIMG_CHECK_ARG(ptrs[i] && ((uintptr_t) ptrs[i] & 3) == 0);
            alignment |= (uintptr_t) ptrs[i];
        }
    }
    if (line) {
        // the line pass reads the median map
        KIMG_CHECK_ARG(out.median && ((uintptr_t) line & 3) == 0);
        KIMG_CHECK_ARG(line_channel_pitch >= plane_elements);
        alignment |= (uintptr_t) line | ((uintptr_t) line_channel_pitch * sizeof(float));
        // in place (the same cube, the same pitch), or two cubes that share no byte
        if (!(line == cube && line_channel_pitch == channel_pitch)) {
            const uintptr_t from = (uintptr_t) cube, to = (uintptr_t) line;
            const uintptr_t from_bytes =
                ((uintptr_t) (num_channels - 1) * channel_pitch + plane_elements) * sizeof(float);
            const uintptr_t to_bytes =
                ((uintptr_t) (num_channels - 1) * line_channel_pitch + plane_elements) * sizeof(float);
            KIMG_CHECK_ARG(from + from_bytes <= to || to + to_bytes <= from);
        }
    }
    if (num_channels > COL_MAX_CHANNELS || !ss_plane_fits(plane_elements))
        return KIMG_EUNSUPPORTED;

    ss_call a = {};
    col_mask filled = {};
    for (int c = 0; c < num_channels; c++) {
        if (!filled_host[c])
            continue;
        col_set(filled, c);
        if (c >= first && c < stop && stat_host[c]) {
            col_set(a.enter, c);
            a.S++;
        }
    }
    if (form == KIMG_SPECTRUM_FORM_RESIDENT && a.S > SS_RESIDENT_LIMIT)
        return KIMG_EUNSUPPORTED;
    if (plane_elements == 0)
        return 0;
    a.cube = cube;
    a.pitch = channel_pitch;
    a.first = first;
    a.stop = stop;
    a.estimator = estimator;
    a.min_samples = min_samples;
    a.resident = form == KIMG_SPECTRUM_FORM_RESIDENT
                 || (form == KIMG_SPECTRUM_FORM_AUTO && a.S <= SS_AUTO_RESIDENT);
    a.stream = (hipStream_t) stream;

    // the form (kimg_cube_column.h): four elements per thread where every address a thread forms is
    // 16-byte aligned, one element per thread for the tail and for everything else
    const int64_t done = col_vector_elements(alignment, plane_elements);
    if (done)
        if (const int rc = ss_launch<4>(a, 0, done / 4, out))
            return rc;
    if (done < plane_elements)
        if (const int rc = ss_launch<1>(a, done, plane_elements - done, ss_offset(out, done)))
            return rc;
    if (line) {
        if (done)
            ss_line_kernel<4><<<col_blocks(done / 4), COL_THREADS, 0, a.stream>>>(
                cube, channel_pitch, line, line_channel_pitch, done / 4, num_channels, filled,
                out.median);
        if (done < plane_elements)
            ss_line_kernel<1><<<col_blocks(plane_elements - done), COL_THREADS, 0, a.stream>>>(
                cube + done, channel_pitch, line + done, line_channel_pitch, plane_elements - done,
                num_channels, filled, out.median + done);
    }
    return kimg_launch_status();
}

KIMG_PRELOAD_THIS_UNIT((ss_line_kernel<1>))
