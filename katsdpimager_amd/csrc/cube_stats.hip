// Cube plane statistics (include/kimg.h, "Cube plane statistics"): for every group -- a channel's
// planes pooled, or one plane -- of a cube [C][P][H][W] the count of finite samples, their min, max
// and median and a robust sigma, by exact selection, all groups at once.  katsdpimager_amd/cube_stats.py
// holds the same contract as numpy (cube_stats_host).
//
// A batched byte-wise radix select, the single-image form of clean.hip (abs_histogram2_kernel,
// radix_select2_kernel) with per-group state.  A pass is two launches whatever C is: cst_pass_kernel,
// grid (workgroups of a group, groups of a channel, channels of the range), adds a workgroup's LDS
// histograms into one of a few global slots of its group; cst_select_kernel, one workgroup a group,
// folds the slots, picks the bin that holds each of the two middle ranks and descends.  The group
// comes from the grid, so `filled`, the prefixes and the ranks are the same for every lane (scalar
// loads) and the skip of an unfilled or empty group is a uniform branch.
//
// Keys.  Values are ordered by key(x) = bits ^ (bits >> 31 ? 0xffffffff : 0x80000000), the monotone
// map of the float32 bit pattern (-0 below +0).  Two selects run side by side, each for the ranks
// (n - 1) / 2 and n / 2: select 0 on key(x) gives the median; select 1 on key(|v|) = 0x80000000 | abs
// bits gives sigma, with v = x ('median_abs') or v = x - m ('mad', m = the median).
//
// Which reads.  'median_abs' runs both selects in the same four passes -- both keys come from the
// same load -- so the cube is read 4 times, not 8: the first pass only makes the histogram of
// key(x)'s top byte (sign and seven exponent bits), and select 1's top histogram follows from it in
// the select step, A[0x80 + b] = S[0x80 + b] + S[0x7f - b].  'mad' needs m first: four passes of
// select 0 alone, then four of select 1: 8 reads.
// The count n is the sum of the first histogram, so the ranks are made on the device and there is no
// host round trip; min and max are taken on the keys in the same pass.
// The top byte of noise-like data takes a few neighbouring values per sign, and 64 LDS atomics on one
// address are served one after the other: a thread counts the four exponent bytes up to the largest
// of its wave's first loads, for either sign, in registers (anything else goes to LDS directly).
//
// A group is E contiguous elements (the plane is dense).  Loads: 16 bytes where the cube's base, the
// channel pitch and W are multiples of 4 floats, one element otherwise.  With neither border nor
// region the element index is all a thread needs (PLAIN); otherwise (y, x) is made from it, once a
// load.
#include "kimg_cube_column.h"

namespace {

constexpr int CST_THREADS = 256;
constexpr int CST_UNROLL = 4;                   // loads a thread has in flight
constexpr int CST_CHUNK = CST_THREADS * CST_UNROLL;     // loads of a workgroup per round
constexpr int CST_MAX_SLOTS = 16;
constexpr int CST_MAX_BLOCKS = 8192;            // workgroups of a pass, about

// mode of a pass: which selects it serves
constexpr int CST_MEDIAN = 0;                   // select 0 alone ('mad', first half)
constexpr int CST_BOTH = 1;                     // selects 0 and 1 on x ('median_abs')
constexpr int CST_DEVIATION = 2;                // select 1 on x - m ('mad', second half)

struct cst_select {
    uint32_t prefix[2];         // bytes of the rank's key chosen so far
    uint32_t k[2];              // rank still to resolve inside the prefix
};

struct cst_group {
    cst_select sel[2];
    uint32_t n;                 // finite samples (0 until the first select step)
    uint32_t max_key, inv_min_key;      // max of key, max of ~key
    uint32_t median;            // bits of m, once select 0 has ended
    uint32_t reserved[4];
};

// Global histogram slots per (group, select, rank): many groups spread the atomics by themselves
inline int cst_slots(int64_t groups)
{
    const int64_t s = 256 / groups;
    return (int) (s < 1 ? 1 : s > CST_MAX_SLOTS ? CST_MAX_SLOTS : s);
}

__host__ __device__ inline size_t cst_hist_index(int64_t group, int select, int rank, int slots, int slot)
{
    return ((((size_t) group * 2 + select) * 2 + rank) * slots + slot) * 256;
}

__device__ inline uint32_t cst_key(uint32_t bits)
{
    return bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u);
}

__device__ inline float cst_value(uint32_t key)
{
    return __uint_as_float((key & 0x80000000u) ? key ^ 0x80000000u : ~key);
}

__device__ inline bool cst_finite(uint32_t bits) { return (bits & 0x7f800000u) != 0x7f800000u; }

__device__ inline bool cst_filled(const col_mask &f, int c) { return (f.bits[c >> 5] >> (c & 31)) & 1u; }

// Zero the scratch; NaN and 0 into every group's outputs
__global__ __launch_bounds__(CST_THREADS)
void cst_init_kernel(uint32_t *__restrict__ scratch, size_t words, int64_t groups,
                     uint32_t *__restrict__ count, float *__restrict__ vmin, float *__restrict__ vmax,
                     float *__restrict__ median, float *__restrict__ sigma)
{
    const size_t stride = (size_t) gridDim.x * CST_THREADS;
    const size_t start = (size_t) blockIdx.x * CST_THREADS + threadIdx.x;
    for (size_t i = start; i < words; i += stride)
        scratch[i] = 0;
    for (size_t i = start; i < (size_t) groups; i += stride) {
        count[i] = 0;
        vmin[i] = col_nan();
        vmax[i] = col_nan();
        median[i] = col_nan();
        sigma[i] = col_nan();
    }
}

// One pass over every group of the range: histograms of byte `shift / 8` of the keys behind each
// rank's prefix.  TOP: the first pass of a select (every finite sample counts; one histogram).
template <int V, bool PLAIN, bool TOP, int MODE>
__global__ __launch_bounds__(CST_THREADS)
void cst_pass_kernel(const float *__restrict__ cube, int64_t pitch, uint32_t E, int H, int W,
                     int border, const uint8_t *__restrict__ region, int G, int first,
                     const col_mask filled, int shift, cst_group *__restrict__ groups,
                     uint32_t *__restrict__ hist, int slots)
{
    // [select][rank][bin]
    __shared__ uint32_t local[2][2][256];
    __shared__ uint32_t extreme[2];
    const int c = first + blockIdx.z;
    if (!cst_filled(filled, c))
        return;
    const int64_t group = (int64_t) c * G + blockIdx.y;
    const cst_group *st = groups + group;
    if ((!TOP || MODE == CST_DEVIATION) && st->n == 0)
        return;
    const int t = threadIdx.x;
    for (int i = t; i < 4 * 256; i += CST_THREADS)
        (&local[0][0][0])[i] = 0;
    if (t < 2)
        extreme[t] = 0;
    const float m = __uint_as_float(st->median);
    const uint32_t p00 = st->sel[0].prefix[0], p01 = st->sel[0].prefix[1];
    const uint32_t p10 = st->sel[1].prefix[0], p11 = st->sel[1].prefix[1];
    const bool split0 = p00 != p01, split1 = p10 != p11;
    __syncthreads();

    const float *src = cube + (int64_t) c * pitch + (int64_t) blockIdx.y * E;
    const int64_t loads = E / V;
    const uint32_t HW = (uint32_t) H * (uint32_t) W;
    uint32_t base = 0, near[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool have_base = false;
    uint32_t kmax = 0, inv_kmin = 0;

    // (the trip count is the workgroup's: the shuffles below see every lane)
    for (int64_t chunk = blockIdx.x; chunk * CST_CHUNK < loads; chunk += gridDim.x) {
        uint32_t bits[CST_UNROLL][V];
        bool ok[CST_UNROLL][V];
#pragma unroll
        for (int u = 0; u < CST_UNROLL; u++) {
            const int64_t l = chunk * CST_CHUNK + u * CST_THREADS + t;
            const bool valid = l < loads;
            float v[V];
#pragma unroll
            for (int i = 0; i < V; i++)
                v[i] = 0.0f;
            if (valid)
                col_load<V>(src + l * V, v);
            bool cand[V];
            if constexpr (PLAIN) {
#pragma unroll
                for (int i = 0; i < V; i++)
                    cand[i] = valid;
            } else {
                // (V = 4: W is a multiple of 4, the four elements share a row)
                const uint32_t e = (uint32_t) (l * V);
                const uint32_t rem = e % HW;
                const int y = (int) (rem / (uint32_t) W);
                const int x = (int) (rem - (uint32_t) y * (uint32_t) W);
                const bool row = valid && y >= border && y < H - border;
#pragma unroll
                for (int i = 0; i < V; i++) {
                    cand[i] = row && x + i >= border && x + i < W - border;
                    if (region && cand[i])
                        cand[i] = region[(int64_t) y * W + x + i] != 0;
                }
            }
#pragma unroll
            for (int i = 0; i < V; i++) {
                bits[u][i] = __float_as_uint(v[i]);
                ok[u][i] = cand[i] && cst_finite(bits[u][i]);
            }
        }
        if constexpr (TOP) {
            if (!have_base) {
                // the largest exponent byte (seven bits: sign-less, >> 24) of the wave's first loads
                const uint32_t b0 = MODE == CST_DEVIATION ? __float_as_uint(__uint_as_float(bits[0][0]) - m)
                                                          : bits[0][0];
                base = ok[0][0] ? (b0 >> 24) & 0x7fu : 0u;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1)
                    base = max(base, (uint32_t) __shfl_xor((int) base, off, WAVE));
                have_base = true;
            }
        }
#pragma unroll
        for (int u = 0; u < CST_UNROLL; u++)
#pragma unroll
            for (int i = 0; i < V; i++) {
                const uint32_t b = bits[u][i];
                const bool on = ok[u][i];
                // select 0: key(x); select 1: key(|v|), v = x or x - m
                const uint32_t key0 = cst_key(b);
                const uint32_t vb = MODE == CST_DEVIATION ? __float_as_uint(__uint_as_float(b) - m) : b;
                const uint32_t key1 = 0x80000000u | vb;
                if constexpr (TOP) {
                    const uint32_t key = MODE == CST_DEVIATION ? key1 : key0;
                    const uint32_t top = key >> 24;
                    const uint32_t exponent = (top & 0x80u) ? top & 0x7fu : 0x7fu - top;
                    const uint32_t d = base - exponent;
                    const uint32_t code = d | ((top & 0x80u) ? 0u : 4u);
                    if (on) {
#pragma unroll
                        for (int j = 0; j < 8; j++)
                            near[j] += (d <= 3u) & (code == (uint32_t) j);
                        if (d > 3u)
                            atomicAdd(&local[MODE == CST_DEVIATION ? 1 : 0][0][top], 1u);
                        if constexpr (MODE != CST_DEVIATION) {
                            kmax = max(kmax, key);
                            inv_kmin = max(inv_kmin, ~key);
                        }
                    }
                } else {
                    if constexpr (MODE != CST_DEVIATION) {
                        const uint32_t upper = key0 >> (shift + 8), bin = (key0 >> shift) & 255u;
                        if (on && upper == p00)
                            atomicAdd(&local[0][0][bin], 1u);
                        if (split0 && on && upper == p01)
                            atomicAdd(&local[0][1][bin], 1u);
                    }
                    if constexpr (MODE != CST_MEDIAN) {
                        const uint32_t upper = key1 >> (shift + 8), bin = (key1 >> shift) & 255u;
                        if (on && upper == p10)
                            atomicAdd(&local[1][0][bin], 1u);
                        if (split1 && on && upper == p11)
                            atomicAdd(&local[1][1][bin], 1u);
                    }
                }
            }
    }
    if constexpr (TOP) {
        // (a counter that is not 0 has base - j >= 0: it counted an exponent byte)
#pragma unroll
        for (int j = 0; j < 8; j++)
            if (near[j]) {
                const uint32_t exponent = base - (uint32_t) (j & 3);
                const uint32_t top = j < 4 ? 0x80u | exponent : 0x7fu - exponent;
                atomicAdd(&local[MODE == CST_DEVIATION ? 1 : 0][0][top], near[j]);
            }
        if constexpr (MODE != CST_DEVIATION) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                kmax = max(kmax, (uint32_t) __shfl_xor((int) kmax, off, WAVE));
                inv_kmin = max(inv_kmin, (uint32_t) __shfl_xor((int) inv_kmin, off, WAVE));
            }
            if ((t & (WAVE - 1)) == 0) {
                atomicMax(&extreme[0], kmax);
                atomicMax(&extreme[1], inv_kmin);
            }
        }
    }
    __syncthreads();
    const int slot = blockIdx.x % slots;
#pragma unroll
    for (int s = 0; s < 2; s++)
#pragma unroll
        for (int r = 0; r < 2; r++)
            if (local[s][r][t])
                atomicAdd(&hist[cst_hist_index(group, s, r, slots, slot) + t], local[s][r][t]);
    if constexpr (TOP && MODE != CST_DEVIATION) {
        if (t == 0 && (extreme[0] | extreme[1])) {
            atomicMax(&groups[group].max_key, extreme[0]);
            atomicMax(&groups[group].inv_min_key, extreme[1]);
        }
    }
}

// Inclusive sum over the workgroup's 256 values, through `cum`
__device__ inline uint32_t cst_scan(uint32_t *cum, uint32_t value)
{
    const int t = threadIdx.x;
    __syncthreads();
    cum[t] = value;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const uint32_t add = t >= off ? cum[t - off] : 0;
        __syncthreads();
        cum[t] += add;
        __syncthreads();
    }
    return cum[t];
}

// The slots of one histogram folded, thread t its bin t, and cleared for the next pass
__device__ inline uint32_t cst_fold(uint32_t *hist, int64_t group, int select, int rank, int slots)
{
    uint32_t total = 0;
    for (int slot = 0; slot < slots; slot++) {
        uint32_t *p = hist + cst_hist_index(group, select, rank, slots, slot) + threadIdx.x;
        total += *p;
        *p = 0;
    }
    return total;
}

// One workgroup a group: for each select of the mode and each of its two ranks the byte whose bin
// holds the rank; TOP makes n and the ranks first.  `last`: the selects end here, write the outputs.
template <bool TOP>
__global__ __launch_bounds__(CST_THREADS)
void cst_select_kernel(cst_group *__restrict__ groups, uint32_t *__restrict__ hist, int slots, int G,
                       int first, const col_mask filled, int mode, bool last, float to_rms,
                       uint32_t *__restrict__ count, float *__restrict__ vmin,
                       float *__restrict__ vmax, float *__restrict__ median, float *__restrict__ sigma)
{
    __shared__ uint32_t cum[256];
    __shared__ uint32_t top[256];
    __shared__ uint32_t chosen[2][2];
    const int c = first + blockIdx.y;
    if (!cst_filled(filled, c))
        return;
    const int64_t group = (int64_t) c * G + blockIdx.x;
    cst_group *st = groups + group;
    const int t = threadIdx.x;
    uint32_t n = st->n;
    if ((!TOP || mode == CST_DEVIATION) && n == 0)
        return;
    uint32_t prefix[2][2], k[2][2];
    for (int s = 0; s < 2; s++)
        for (int r = 0; r < 2; r++) {
            prefix[s][r] = st->sel[s].prefix[r];
            k[s][r] = st->sel[s].k[r];
        }
    const int s_first = mode == CST_DEVIATION ? 1 : 0, s_last = mode == CST_MEDIAN ? 0 : 1;

    if constexpr (TOP) {
        const uint32_t mine = cst_fold(hist, group, s_first, 0, slots);
        uint32_t inclusive = cst_scan(cum, mine);
        n = cum[255];
        if (n == 0)
            return;                 // (the outputs are the init's: NaN and 0)
        top[t] = mine;
        for (int s = s_first; s <= s_last; s++) {
            uint32_t here = mine;
            if (s == 1 && mode == CST_BOTH) {
                // key(|x|)'s top byte from key(x)'s: 0x80 + b holds +b and -b
                __syncthreads();
                here = t >= 128 ? top[t] + top[255 - t] : 0u;
                inclusive = cst_scan(cum, here);
            }
            const uint32_t below = inclusive - here;
            for (int r = 0; r < 2; r++) {
                const uint32_t rank = r == 0 ? (n - 1) / 2 : n / 2;
                if (below <= rank && rank < inclusive) {        // exactly one bin
                    st->sel[s].k[r] = rank - below;
                    st->sel[s].prefix[r] = (uint32_t) t;
                }
            }
        }
        if (t == 0)
            st->n = n;
    } else {
        for (int s = s_first; s <= s_last; s++) {
            const bool split = prefix[s][0] != prefix[s][1];
            uint32_t here = 0, inclusive = 0;
            for (int r = 0; r < 2; r++) {
                if (r == 0 || split) {
                    here = cst_fold(hist, group, s, r, slots);
                    inclusive = cst_scan(cum, here);
                }
                const uint32_t below = inclusive - here;
                if (below <= k[s][r] && k[s][r] < inclusive) {  // exactly one bin
                    const uint32_t now = (prefix[s][r] << 8) | (uint32_t) t;
                    st->sel[s].k[r] = k[s][r] - below;
                    st->sel[s].prefix[r] = now;
                    chosen[s][r] = now;
                }
            }
        }
        if (last) {
            __syncthreads();
            if (t == 0) {
                if (mode != CST_DEVIATION) {
                    const float lo = cst_value(chosen[0][0]), hi = cst_value(chosen[0][1]);
                    const float mid = (lo + hi) / 2.0f;
                    st->median = __float_as_uint(mid);
                    count[group] = n;
                    vmin[group] = cst_value(~st->inv_min_key);
                    vmax[group] = cst_value(st->max_key);
                    median[group] = mid;
                }
                if (mode != CST_MEDIAN) {
                    const float lo = cst_value(chosen[1][0]), hi = cst_value(chosen[1][1]);
                    const float mid = (lo + hi) / 2.0f;
                    sigma[group] = mid * to_rms;
                }
            }
        }
    }
}

struct cst_call {
    const float *cube;
    int64_t pitch;
    uint32_t E;
    int H, W, border;
    const uint8_t *region;
    int G, first, channels;
    col_mask filled;
    cst_group *groups;
    uint32_t *hist;
    int slots;
    unsigned blocks;
    bool vector, plain;
    hipStream_t stream;
};

template <int V, bool PLAIN, bool TOP, int MODE> void cst_pass_as(const cst_call &a, int shift)
{
    const dim3 grid(a.blocks, (unsigned) a.G, (unsigned) a.channels);
    cst_pass_kernel<V, PLAIN, TOP, MODE><<<grid, CST_THREADS, 0, a.stream>>>(
        a.cube, a.pitch, a.E, a.H, a.W, a.border, a.region, a.G, a.first, a.filled, shift, a.groups,
        a.hist, a.slots);
}

template <bool TOP, int MODE> void cst_pass(const cst_call &a, int shift)
{
    if (a.vector)
        a.plain ? cst_pass_as<4, true, TOP, MODE>(a, shift) : cst_pass_as<4, false, TOP, MODE>(a, shift);
    else
        a.plain ? cst_pass_as<1, true, TOP, MODE>(a, shift) : cst_pass_as<1, false, TOP, MODE>(a, shift);
}

// The four passes of one mode, a pass and a select step each
template <int MODE> void cst_select(const cst_call &a, float to_rms, uint32_t *count, float *vmin,
                                    float *vmax, float *median, float *sigma)
{
    const dim3 grid((unsigned) a.G, (unsigned) a.channels);
    // (the first pass of 'median_abs' is that of the median alone: select 1's histogram follows from it)
    cst_pass<true, MODE == CST_BOTH ? CST_MEDIAN : MODE>(a, 24);
    cst_select_kernel<true><<<grid, CST_THREADS, 0, a.stream>>>(
        a.groups, a.hist, a.slots, a.G, a.first, a.filled, MODE, false, to_rms, count, vmin, vmax,
        median, sigma);
    for (int shift = 16; shift >= 0; shift -= 8) {
        cst_pass<false, MODE>(a, shift);
        cst_select_kernel<false><<<grid, CST_THREADS, 0, a.stream>>>(
            a.groups, a.hist, a.slots, a.G, a.first, a.filled, MODE, shift == 0, to_rms, count, vmin,
            vmax, median, sigma);
    }
}

size_t cst_state_bytes(int64_t groups) { return (size_t) groups * sizeof(cst_group); }

}  // namespace

extern "C" size_t kimg_cube_stats_scratch_bytes(int num_channels, int groups_per_channel)
{
    if (num_channels < 1 || num_channels > COL_MAX_CHANNELS || groups_per_channel < 1
            || groups_per_channel > 65535)
        return 0;
    const int64_t groups = (int64_t) num_channels * groups_per_channel;
    return cst_state_bytes(groups) + cst_hist_index(groups, 0, 0, cst_slots(groups), 0) * sizeof(uint32_t);
}

extern "C" int kimg_cube_stats(const float *cube, int64_t channel_pitch, int num_channels,
                               int num_polarizations, int height, int width,
                               const uint8_t *filled_host, int first, int stop,
                               int pool_polarizations, int estimator, int border,
                               const uint8_t *region, void *scratch, uint32_t *count, float *min,
                               float *max, float *median, float *sigma, void *stream)
{
    KIMG_CHECK_ARG(cube && filled_host && scratch && count && min && max && median && sigma);
    KIMG_CHECK_ARG(num_channels >= 1 && num_channels <= COL_MAX_CHANNELS);
    KIMG_CHECK_ARG(num_polarizations >= 1 && height >= 1 && width >= 1);
    KIMG_CHECK_ARG(first >= 0 && first < stop && stop <= num_channels);
    KIMG_CHECK_ARG(estimator == KIMG_CUBE_STATS_MEDIAN_ABS || estimator == KIMG_CUBE_STATS_MAD);
    KIMG_CHECK_ARG(border >= 0 && 2 * (int64_t) border < (height < width ? height : width));
    KIMG_CHECK_ARG(((uintptr_t) cube & 3) == 0 && ((uintptr_t) scratch & 7) == 0);
    KIMG_CHECK_ARG((((uintptr_t) count | (uintptr_t) min | (uintptr_t) max | (uintptr_t) median
                     | (uintptr_t) sigma) & 3) == 0);
    // (a channel, the cube's extent in bytes and every index the kernels form stay inside int64)
    const int64_t pixels = (int64_t) height * width;
    KIMG_CHECK_ARG(num_polarizations <= INT64_MAX / 8 / pixels);
    const int64_t M = num_polarizations * pixels;
    KIMG_CHECK_ARG(channel_pitch >= M);
    KIMG_CHECK_ARG(channel_pitch <= (INT64_MAX / (int64_t) sizeof(float) - M) / num_channels);
    const bool pool = pool_polarizations != 0;
    const int G = pool ? 1 : num_polarizations;
    const int64_t E = pool ? M : pixels;
    // a group's elements, and with them its candidates and every count, fit 32 bits
    if (E >= ((int64_t) 1 << 32) || G > 65535)
        return KIMG_EUNSUPPORTED;

    cst_call a = {};
    a.cube = cube;
    a.pitch = channel_pitch;
    a.E = (uint32_t) E;
    a.H = height;
    a.W = width;
    a.border = border;
    a.region = region;
    a.G = G;
    a.first = first;
    a.channels = stop - first;
    int active = 0;
    for (int c = first; c < stop; c++)
        if (filled_host[c]) {
            col_set(a.filled, c);
            active++;
        }
    const int64_t groups = (int64_t) num_channels * G;
    a.groups = static_cast<cst_group *>(scratch);
    a.hist = reinterpret_cast<uint32_t *>(static_cast<char *>(scratch) + cst_state_bytes(groups));
    a.slots = cst_slots(groups);
    const uintptr_t alignment = (uintptr_t) cube | ((uintptr_t) channel_pitch * sizeof(float))
                                | ((uintptr_t) width * sizeof(float));
    a.vector = (alignment & 15) == 0;
    a.plain = border == 0 && !region;
    a.stream = (hipStream_t) stream;
    const size_t words = kimg_cube_stats_scratch_bytes(num_channels, G) / sizeof(uint32_t);
    const size_t init = (words + CST_THREADS - 1) / CST_THREADS;
    cst_init_kernel<<<(unsigned) (init < 4096 ? init : 4096), CST_THREADS, 0, a.stream>>>(
        static_cast<uint32_t *>(scratch), words, groups, count, min, max, median, sigma);
    if (active) {
        const int64_t loads = E / (a.vector ? 4 : 1);
        const int64_t cap = CST_MAX_BLOCKS / ((int64_t) active * G);
        const int64_t want = (loads + CST_CHUNK - 1) / CST_CHUNK;
        a.blocks = (unsigned) (want < 1 || cap < 1 ? 1 : want < cap ? want : cap);
        const float to_rms = KIMG_CUBE_STATS_TO_RMS;
        if (estimator == KIMG_CUBE_STATS_MEDIAN_ABS) {
            cst_select<CST_BOTH>(a, to_rms, count, min, max, median, sigma);
        } else {
            cst_select<CST_MEDIAN>(a, to_rms, count, min, max, median, sigma);
            cst_select<CST_DEVIATION>(a, to_rms, count, min, max, median, sigma);
        }
    }
    return kimg_launch_status();
}

KIMG_PRELOAD_THIS_UNIT(cst_init_kernel)
