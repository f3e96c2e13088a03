// Fold pre-pass of the window gridder: runs of consecutive records with equal (u, v, sub_u, sub_v,
// w_plane) become ONE record with the float32 sum of their raw samples (kimg_fold_runs, include/kimg.h).
//
// All records of a run read the same density-weight cell and apply the same rank-1 matrix, so the
// window kernel (grid_mfma.hip) can weight the sum, w * sum(v), where it would have summed the
// weighted samples: it needs no new arithmetic, and the pre-pass no weight gather.  An uncompressed
// track stream repeats its predecessor's sub-cell in 6 of 7 records; building those records inside
// the window kernel costs issue slots that it shares with its matrix instructions, at 3 waves per
// SIMD.  Here the same work is a memory stream: 256-thread workgroups at full occupancy, 10 bytes
// per record read in the first launch, 10 + 8 P in the second.
//
// Two launches, no scan kernel, and NO workgroup ever waits for another one:
//  * the stream is cut into at most 768 contiguous spans of whole tiles (a tile = 256 threads x 8
//    records), one workgroup per span;
//  * launch 1 counts the heads of runs in every span (a span's first record always heads a run:
//    runs are cut at span boundaries, and only there);
//  * launch 2: every workgroup sums the counts of the spans before its own (at most 1024 words) and
//    walks its span tile by tile, carrying the output offset and the open run's partial sum from
//    tile to tile.  Heads and sums are written in stream order: the output is deterministic.
//    Every workgroup also sums ALL counts to H and takes the same decision from it: with
//    2 H > N or H above the output's capacity the header says use_folded = 0 and no record is
//    written -- a stream without duplicates costs the count pass only.
// No allocation, no read-back, no synchronisation: the call is asynchronous and capturable.
//
// A fold plan (kimg_fold_plan) is launch 1 run ahead of time and kept by the caller: the counts
// depend on uv and w_plane alone, which stay the same from one gridding pass over a slice to the
// next.  A call that is given one issues launch 2 only.  The plan is untrusted: launch 2 counts every
// span's heads anyway, and the last workgroup to finish -- found by a ticket, nobody waits -- sets
// use_folded only if every span found the count the plan gave it.  Then the offsets were the right
// ones and the output is what the two launches write; else the window kernel grids the caller's
// stream.  Output indices are checked against the capacity whatever the plan holds.
//
// A fold map (kimg_fold_map) keeps the rest of what uv and w_plane decide: every thread's heads, one
// byte per 8 records, and the compacted coordinates.  A call that is given one reads the samples
// and the head bits and writes the sums -- launch 2 with its key loads, comparisons and coordinate
// stores compiled out, so the sums are added in the same order.  The map is checked when it is made,
// span by span like a plan, and believed afterwards: it belongs to the bytes it was made from.
#include "kimg_record_stream.h"

namespace {

constexpr int FOLD_THREADS = 256;
constexpr int FOLD_RECORDS = 8;                             // consecutive records per thread
constexpr int FOLD_TILE = FOLD_THREADS * FOLD_RECORDS;
constexpr int FOLD_MAX_SPANS = 1024;                        // (what the counts' array holds)
constexpr int FOLD_WAVES = FOLD_THREADS / WAVE;

// workspace layout: header, the spans' counts, then the compacted uv, vis and w_plane
constexpr size_t FOLD_HEADER_BYTES = 256;
constexpr size_t FOLD_COUNTS_BYTES = FOLD_MAX_SPANS * sizeof(uint32_t);
static_assert(sizeof(kimg_fold_header) <= FOLD_HEADER_BYTES && FOLD_COUNTS_BYTES % 256 == 0,
              "the header and the counts are the workspace's first two sections, at 0 and 256");

struct fold_ws {
    kimg_fold_header *header;
    uint32_t *counts;
    int2 *uv;
    float2 *vis;
    int16_t *w_plane;
    size_t total;
};

// (`workspace` null: the size only)
inline fold_ws fold_carve(int P, int64_t capacity, void *workspace)
{
    const size_t cap = capacity > 0 ? (size_t) capacity : 0;
    ws_carver c(workspace);
    fold_ws ws;
    ws.header = reinterpret_cast<kimg_fold_header *>(c.take<unsigned char>(FOLD_HEADER_BYTES));
    ws.counts = c.take<uint32_t>(FOLD_COUNTS_BYTES / sizeof(uint32_t));
    ws.uv = c.take<int2>(cap);
    ws.vis = c.take<float2>(cap * P);
    ws.w_plane = c.take<int16_t>(cap);
    ws.total = c.total();
    return ws;
}

struct fold_plan {
    int spans;
    int64_t tiles_per_span;
};

// As many spans as workgroups of the compaction kernel are resident at once on 256 CUs -- three per
// CU at the 132 (P = 1) and 139 (P = 2) registers it takes, two with more polarizations -- so that
// a launch is one round of workgroups of equal length.
inline fold_plan fold_plan_of(int64_t num_vis, int P)
{
    const int max_spans = P <= 2 ? 768 : 512;
    static_assert(768 <= FOLD_MAX_SPANS, "the counts' array holds one word per span");
    const int64_t tiles = (num_vis + FOLD_TILE - 1) / FOLD_TILE;
    fold_plan p;
    p.tiles_per_span = (tiles + max_spans - 1) / max_spans;
    p.spans = (int) ((tiles + p.tiles_per_span - 1) / p.tiles_per_span);
    return p;
}

// A fold map's sections behind its kimg_fold_map_data: the head bits, one byte per thread and tile,
// then the compacted uv and w_plane.  Where w_plane begins depends on H alone, which both the launch
// that fills a map and the pass that uses it sum from the same counts.
__host__ __device__ inline size_t fold_map_bits_bytes(int64_t num_vis)
{
    return ((size_t) (num_vis + FOLD_RECORDS - 1) / FOLD_RECORDS + 15) & ~(size_t) 15;
}

__host__ __device__ inline int64_t fold_map_round(int64_t heads) { return (heads + 7) & ~(int64_t) 7; }

__host__ __device__ inline const uint8_t *fold_map_bits(const kimg_fold_map_data *map)
{
    return reinterpret_cast<const uint8_t *>(map + 1);
}

__host__ __device__ inline const int2 *fold_map_uv(const kimg_fold_map_data *map, int64_t num_vis)
{
    return reinterpret_cast<const int2 *>(fold_map_bits(map) + fold_map_bits_bytes(num_vis));
}

__host__ __device__ inline const int16_t *fold_map_w(const kimg_fold_map_data *map, int64_t num_vis,
                                                     int64_t H)
{
    return reinterpret_cast<const int16_t *>(fold_map_uv(map, num_vis) + fold_map_round(H));
}

inline size_t fold_map_bytes(int64_t num_vis, int64_t heads)
{
    return sizeof(kimg_fold_map_data) + fold_map_bits_bytes(num_vis)
           + (size_t) fold_map_round(heads) * (sizeof(int2) + sizeof(int16_t));
}

// The keys of a thread's 8 records [i0, i0 + 8) and of the record before them
struct fold_keys {
    int2 uv[FOLD_RECORDS];
    int wp[FOLD_RECORDS];
    int2 prev_uv;
    int prev_wp;
    unsigned heads;                 // (a fold map's pass: fold_heads as the map keeps it, no keys)
};

// (uv, w_plane 16-byte aligned; i0 a multiple of 8: whole 16-byte words while the thread's records
// all exist, single clamped loads at the stream's end)
__device__ __attribute__((always_inline)) inline void fold_load_keys(
    const int16_t *__restrict__ uv, const int16_t *__restrict__ w_plane, int64_t i0, int64_t num_vis,
    int64_t span_start, fold_keys &k)
{
    if (i0 + FOLD_RECORDS <= num_vis) {
        const int4 *u4 = reinterpret_cast<const int4 *>(uv + 4 * i0);
#pragma unroll
        for (int j = 0; j < FOLD_RECORDS / 2; j++) {
            const int4 t = u4[j];
            k.uv[2 * j] = make_int2(t.x, t.y);
            k.uv[2 * j + 1] = make_int2(t.z, t.w);
        }
        const int4 w4 = *reinterpret_cast<const int4 *>(w_plane + i0);
        const int w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            k.wp[2 * j] = (short) (w[j] & 0xffff);
            k.wp[2 * j + 1] = w[j] >> 16;
        }
    } else {
#pragma unroll
        for (int j = 0; j < FOLD_RECORDS; j++) {
            int64_t i = i0 + j;
            i = i < num_vis ? i : num_vis - 1;
            k.uv[j] = reinterpret_cast<const int2 *>(uv)[i];
            k.wp[j] = w_plane[i];
        }
    }
    k.prev_uv = k.uv[0];
    k.prev_wp = k.wp[0];
    if (i0 > span_start && i0 < num_vis) {
        k.prev_uv = reinterpret_cast<const int2 *>(uv)[i0 - 1];
        k.prev_wp = w_plane[i0 - 1];
    }
}

// bit j: record i0 + j exists and heads a run
__device__ __attribute__((always_inline)) inline unsigned fold_heads(
    const fold_keys &k, int64_t i0, int64_t num_vis, int64_t span_start)
{
    unsigned heads = 0;
#pragma unroll
    for (int j = 0; j < FOLD_RECORDS; j++) {
        const int2 puv = j ? k.uv[j - 1] : k.prev_uv;
        const int pwp = j ? k.wp[j - 1] : k.prev_wp;
        const bool differs = k.uv[j].x != puv.x || k.uv[j].y != puv.y || k.wp[j] != pwp;
        const bool head = i0 + j < num_vis && (i0 + j == span_start || differs);
        heads |= head ? 1u << j : 0u;
    }
    return heads;
}

// sum over the workgroup, valid in every thread (s_red: FOLD_WAVES words; ends with a barrier, so
// that s_red can be used again at once)
__device__ inline unsigned long long fold_block_sum(unsigned long long v, unsigned long long *s_red)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_xor(v, off, WAVE);
    if ((threadIdx.x & 63) == 0)
        s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long sum = 0;
#pragma unroll
    for (int w = 0; w < FOLD_WAVES; w++)
        sum += s_red[w];
    __syncthreads();
    return sum;
}

__global__ __launch_bounds__(FOLD_THREADS) void fold_count_kernel(
    const int16_t *__restrict__ uv, const int16_t *__restrict__ w_plane, int64_t num_vis,
    int64_t tiles_per_span, uint32_t *__restrict__ counts)
{
    __shared__ unsigned long long s_red[FOLD_WAVES];
    const int64_t span_start = (int64_t) blockIdx.x * tiles_per_span * FOLD_TILE;
    int64_t span_end = span_start + tiles_per_span * FOLD_TILE;
    span_end = span_end < num_vis ? span_end : num_vis;
    unsigned count = 0;
#pragma unroll 2
    for (int64_t tile = span_start; tile < span_end; tile += FOLD_TILE) {
        const int64_t i0 = tile + (int64_t) threadIdx.x * FOLD_RECORDS;
        if (i0 < num_vis) {
            fold_keys k;
            fold_load_keys(uv, w_plane, i0, num_vis, span_start, k);
            count += __builtin_popcount(fold_heads(k, i0, num_vis, span_start));
        }
    }
    const unsigned long long sum = fold_block_sum(count, s_red);
    if (threadIdx.x == 0)
        counts[blockIdx.x] = (uint32_t) sum;
}

// A fold plan's fields from the counts that fold_count_kernel left in it (one workgroup)
__global__ __launch_bounds__(FOLD_THREADS) void fold_plan_finish_kernel(
    kimg_fold_plan_data *__restrict__ plan, int64_t num_vis, int64_t tiles_per_span, int spans)
{
    __shared__ unsigned long long s_red[FOLD_WAVES];
    unsigned long long all = 0;
    for (int i = threadIdx.x; i < KIMG_FOLD_MAX_SPANS; i += FOLD_THREADS) {
        if (i < spans)
            all += plan->counts[i];
        else
            plan->counts[i] = 0;
    }
    const unsigned long long H = fold_block_sum(all, s_red);
    if (threadIdx.x == 0) {
        plan->magic = KIMG_FOLD_PLAN_MAGIC;
        plan->spans = (uint32_t) spans;
        plan->num_vis = num_vis;
        plan->tiles_per_span = tiles_per_span;
        plan->count = (int64_t) H;
    }
    if (threadIdx.x < 8)
        plan->reserved[threadIdx.x] = 0;
}

// What the segmented scan over a tile's threads carries: heads seen, whether any, and the sum of the
// samples since the last head (of all samples while there was none)
template <int P>
struct fold_elem {
    int cnt, flag;
    float2 s[P];
};

template <int P>
__device__ __attribute__((always_inline)) inline fold_elem<P> fold_combine(
    const fold_elem<P> &a, const fold_elem<P> &b)         // a: the earlier records
{
    fold_elem<P> r;
    r.cnt = a.cnt + b.cnt;
    r.flag = a.flag | b.flag;
#pragma unroll
    for (int p = 0; p < P; p++) {
        r.s[p].x = b.flag ? b.s[p].x : a.s[p].x + b.s[p].x;
        r.s[p].y = b.flag ? b.s[p].y : a.s[p].y + b.s[p].y;
    }
    return r;
}

template <int P>
__device__ __attribute__((always_inline)) inline fold_elem<P> fold_shfl_up(const fold_elem<P> &e, int d)
{
    fold_elem<P> r;
    r.cnt = __shfl_up(e.cnt, d, WAVE);
    r.flag = __shfl_up(e.flag, d, WAVE);
#pragma unroll
    for (int p = 0; p < P; p++) {
        r.s[p].x = __shfl_up(e.s[p].x, d, WAVE);
        r.s[p].y = __shfl_up(e.s[p].y, d, WAVE);
    }
    return r;
}

// A thread's samples of one tile
template <int P>
struct fold_samples {
    float2 v[FOLD_RECORDS][P];
};

template <int P>
__device__ __attribute__((always_inline)) inline void fold_load_samples(
    const float2 *__restrict__ vis, int64_t i0, int64_t num_vis, fold_samples<P> &s)
{
    if (i0 + FOLD_RECORDS <= num_vis) {
        // 8 P complex samples = 4 P words of 16 bytes
        const float4 *v4 = reinterpret_cast<const float4 *>(vis + i0 * P);
#pragma unroll
        for (int j = 0; j < FOLD_RECORDS * P / 2; j++) {
            const float4 t = v4[j];
            s.v[(2 * j) / P][(2 * j) % P] = make_float2(t.x, t.y);
            s.v[(2 * j + 1) / P][(2 * j + 1) % P] = make_float2(t.z, t.w);
        }
    } else {
#pragma unroll
        for (int j = 0; j < FOLD_RECORDS; j++) {
            int64_t i = i0 + j;
            i = i < num_vis ? i : num_vis - 1;
#pragma unroll
            for (int p = 0; p < P; p++)
                s.v[j][p] = vis[i * P + p];
        }
    }
}

// PLANNED: `counts` are a fold plan's (`plan`, untrusted device data) and not this call's count
// launch's.  A plan made for another length or layout is refused by every workgroup alike; counts
// of any value give offsets in [0, H] with H <= capacity, and every store below checks its index
// against the capacity.  Each workgroup leaves its own count of heads in `recount` and, with a
// ticket, whether it was the plan's; the last one to finish writes use_folded.
//
// MAPPED: `counts` are a fold map's (`map`, untrusted device data as well), and so are the heads: no
// key is loaded or compared and no coordinate stored -- the header points at the map's.  All else is
// the one body: the sums of the samples are added in the order of the unmapped forms, so out_vis is
// theirs bit for bit.  A map was checked span by span when it was made (`valid`, fold_map_kernel);
// one that is not valid, or is another length's or layout's, is refused by every workgroup alike.
// Its head bits are believed: wrong ones give wrong sums, at indices that every store still checks
// against the capacity.
template <int P, bool PLANNED, bool MAPPED>
__global__ __launch_bounds__(FOLD_THREADS) void fold_compact_kernel(
    const int16_t *__restrict__ uv, const int16_t *__restrict__ w_plane,
    const float2 *__restrict__ vis, int64_t num_vis, int64_t tiles_per_span, int spans,
    const uint32_t *__restrict__ counts, int64_t capacity, kimg_fold_header *__restrict__ header,
    int2 *__restrict__ out_uv, int16_t *__restrict__ out_w, float2 *__restrict__ out_vis,
    const kimg_fold_plan_data *__restrict__ plan, uint32_t *__restrict__ recount,
    const kimg_fold_map_data *__restrict__ map)
{
    static_assert(!(PLANNED && MAPPED), "a map holds its plan's counts, checked when it was made");
    __shared__ unsigned long long s_red[FOLD_WAVES];
    __shared__ fold_elem<P> s_tot[2][FOLD_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    bool plan_ok = true;
    if (PLANNED)
        plan_ok = plan->magic == KIMG_FOLD_PLAN_MAGIC && plan->spans == (uint32_t) spans
                  && plan->num_vis == num_vis && plan->tiles_per_span == tiles_per_span;
    if (MAPPED)
        plan_ok = map->magic == KIMG_FOLD_MAP_MAGIC && map->valid == 1u
                  && map->spans == (uint32_t) spans && map->num_vis == num_vis
                  && map->tiles_per_span == tiles_per_span;
    // the records before this span, and all of them: every workgroup reads the same counts and
    // takes the same decision
    unsigned long long before = 0, all = 0;
    for (int i = threadIdx.x; i < spans; i += FOLD_THREADS) {
        const unsigned c = counts[i];
        all += c;
        before += i < (int) blockIdx.x ? c : 0u;
    }
    const int64_t offset = (int64_t) fold_block_sum(before, s_red);
    const int64_t H = (int64_t) fold_block_sum(all, s_red);
    bool use = plan_ok && 2 * H <= num_vis && H <= capacity;
    if (MAPPED)                     // (the sum its maker wrote: where the map's w_plane begins)
        use = use && map->count == H;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (!PLANNED || !use)       // (a plan's verdict comes with the last ticket)
            header->use_folded = use ? 1u : 0u;
        header->spans = (uint32_t) spans;
        header->count = H;
        if (MAPPED) {
            header->uv = reinterpret_cast<const int16_t *>(fold_map_uv(map, num_vis));
            header->w_plane = fold_map_w(map, num_vis, H);
        } else {
            header->uv = reinterpret_cast<const int16_t *>(out_uv);
            header->w_plane = out_w;
        }
        header->vis = out_vis;
        header->capacity = capacity;
    }
    if (!use)
        return;

    const int64_t span_start = (int64_t) blockIdx.x * tiles_per_span * FOLD_TILE;
    int64_t span_end = span_start + tiles_per_span * FOLD_TILE;
    span_end = span_end < num_vis ? span_end : num_vis;
    // a tile's loads are issued before the tile before it is worked on (one polarization, and two
    // without the keys: with more the second set of registers would cost a wave per SIMD)
    constexpr bool PREFETCH = P == 1 || (MAPPED && P == 2);
    fold_keys keys, next_keys;
    fold_samples<P> smp, next_smp;
    const uint8_t *__restrict__ map_bits = MAPPED ? fold_map_bits(map) : nullptr;
    auto load_tile = [&](int64_t tile, fold_keys &k, fold_samples<P> &s) __attribute__((always_inline)) {
        const int64_t i0 = tile + (int64_t) threadIdx.x * FOLD_RECORDS;
        if (tile < span_end && i0 < num_vis) {
            if (MAPPED)
                k.heads = map_bits[i0 / FOLD_RECORDS];
            else
                fold_load_keys(uv, w_plane, i0, num_vis, span_start, k);
            fold_load_samples<P>(vis, i0, num_vis, s);
        }
    };
    if (PREFETCH)
        load_tile(span_start, keys, smp);

    float2 carry[P];                // sum of the run that is open at the end of the tiles so far
#pragma unroll
    for (int p = 0; p < P; p++)
        carry[p] = make_float2(0.0f, 0.0f);
    int64_t run_base = offset;      // output index of the next tile's first head
    int parity = 0;
    for (int64_t tile = span_start; tile < span_end; tile += FOLD_TILE, parity ^= 1) {
        const int64_t i0 = tile + (int64_t) threadIdx.x * FOLD_RECORDS;
        if (PREFETCH)
            load_tile(tile + FOLD_TILE, next_keys, next_smp);
        else
            load_tile(tile, keys, smp);
        const unsigned heads = i0 >= num_vis ? 0u
            : MAPPED ? keys.heads : fold_heads(keys, i0, num_vis, span_start);
        // this thread's element: its heads and the sum since its last head
        fold_elem<P> e;
        e.cnt = __builtin_popcount(heads);
        e.flag = heads != 0;
#pragma unroll
        for (int p = 0; p < P; p++)
            e.s[p] = make_float2(0.0f, 0.0f);
#pragma unroll
        for (int j = 0; j < FOLD_RECORDS; j++) {
            const bool valid = i0 + j < num_vis, head = (heads >> j) & 1u;
#pragma unroll
            for (int p = 0; p < P; p++) {
                const float2 v = valid ? smp.v[j][p] : make_float2(0.0f, 0.0f);
                e.s[p].x = head ? v.x : e.s[p].x + v.x;
                e.s[p].y = head ? v.y : e.s[p].y + v.y;
            }
        }
        // inclusive scan over the wave, the waves' totals through LDS
        fold_elem<P> inc = e;
#pragma unroll
        for (int d = 1; d < WAVE; d *= 2) {
            const fold_elem<P> o = fold_shfl_up<P>(inc, d);
            if (lane >= d)
                inc = fold_combine<P>(o, inc);
        }
        if (lane == WAVE - 1)
            s_tot[parity][wave] = inc;
        fold_elem<P> in = fold_shfl_up<P>(inc, 1);  // what precedes this thread in its wave
        if (lane == 0) {
            in.cnt = in.flag = 0;
#pragma unroll
            for (int p = 0; p < P; p++)
                in.s[p] = make_float2(0.0f, 0.0f);
        }
        __syncthreads();        // (one per tile: s_tot alternates between two copies)
        fold_elem<P> prefix;    // what precedes this thread's wave: earlier tiles' open run, earlier waves
        prefix.cnt = prefix.flag = 0;
#pragma unroll
        for (int p = 0; p < P; p++)
            prefix.s[p] = carry[p];
        fold_elem<P> whole = prefix;
#pragma unroll
        for (int w = 0; w < FOLD_WAVES; w++) {
            whole = fold_combine<P>(whole, s_tot[parity][w]);
            if (w + 1 == wave)
                prefix = whole;
        }
        in = fold_combine<P>(prefix, in);

        // walk the records: a head closes the run before it (writes its sum) and opens its own
        float2 acc[P];
#pragma unroll
        for (int p = 0; p < P; p++)
            acc[p] = in.s[p];
        int64_t r = run_base + in.cnt;
#pragma unroll
        for (int j = 0; j < FOLD_RECORDS; j++) {
            const bool valid = i0 + j < num_vis, head = (heads >> j) & 1u;
            if (head) {
                if (r > offset && r <= capacity)
#pragma unroll
                    for (int p = 0; p < P; p++)
                        out_vis[(r - 1) * P + p] = acc[p];
                if (!MAPPED && r < capacity) {
                    out_uv[r] = keys.uv[j];
                    out_w[r] = (int16_t) keys.wp[j];
                }
                r++;
            }
#pragma unroll
            for (int p = 0; p < P; p++) {
                const float2 v = valid ? smp.v[j][p] : make_float2(0.0f, 0.0f);
                acc[p].x = head ? v.x : acc[p].x + v.x;
                acc[p].y = head ? v.y : acc[p].y + v.y;
            }
        }
        run_base += whole.cnt;
#pragma unroll
        for (int p = 0; p < P; p++)
            carry[p] = whole.s[p];
        if (PREFETCH) {
            keys = next_keys;
            smp = next_smp;
        }
    }
    // the span's last run ends with the span
    if (threadIdx.x == 0 && run_base > offset && run_base <= capacity)
#pragma unroll
        for (int p = 0; p < P; p++)
            out_vis[(run_base - 1) * P + p] = carry[p];
    if (PLANNED && threadIdx.x == 0) {
        const int64_t mine = run_base - offset;
        recount[blockIdx.x] = (uint32_t) mine;
        const unsigned add = 1u + (mine != (int64_t) counts[blockIdx.x] ? 0x10000u : 0u);
        const unsigned now = atomicAdd(&header->ticket[0], add) + add;
        // (the next launch reads the header: no other workgroup of this one does)
        if ((now & 0xffffu) == (unsigned) spans)
            header->use_folded = (now >> 16) == 0 ? 1u : 0u;
    }
}

// Fills a fold map from a stream and its plan: the span layout, offsets and ticket of the planned
// compaction, without the samples.  Every thread leaves its fold_heads, every head its coordinates
// at the index the compaction gives it -- checked against `heads_room`, the records the buffer
// holds, whatever the plan says.  `valid` becomes 1 only when the plan was this layout's, its H fits
// the buffer and every span counted what the plan gave it: a stale plan makes a map that no call
// will use.  (map->ticket zeroed ahead of the launch.)
__global__ __launch_bounds__(FOLD_THREADS) void fold_map_kernel(
    const int16_t *__restrict__ uv, const int16_t *__restrict__ w_plane, int64_t num_vis,
    int64_t tiles_per_span, int spans, const kimg_fold_plan_data *__restrict__ plan,
    int64_t heads_room, kimg_fold_map_data *__restrict__ map)
{
    __shared__ unsigned long long s_red[FOLD_WAVES];
    __shared__ int s_cnt[2][FOLD_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    const bool plan_ok = plan->magic == KIMG_FOLD_PLAN_MAGIC && plan->spans == (uint32_t) spans
                         && plan->num_vis == num_vis && plan->tiles_per_span == tiles_per_span;
    unsigned long long before = 0, all = 0;
    for (int i = threadIdx.x; i < spans; i += FOLD_THREADS) {
        const unsigned c = plan->counts[i];
        all += c;
        before += i < (int) blockIdx.x ? c : 0u;
    }
    const int64_t offset = (int64_t) fold_block_sum(before, s_red);
    const int64_t H = (int64_t) fold_block_sum(all, s_red);
    const bool ok = plan_ok && H <= heads_room;
    if (blockIdx.x == 0) {
        for (int i = threadIdx.x; i < KIMG_FOLD_MAX_SPANS; i += FOLD_THREADS)
            map->counts[i] = i < spans ? plan->counts[i] : 0u;
        if (threadIdx.x == 0) {
            map->magic = KIMG_FOLD_MAP_MAGIC;
            map->spans = (uint32_t) spans;
            map->num_vis = num_vis;
            map->tiles_per_span = tiles_per_span;
            map->count = H;
            map->heads = heads_room;
            map->reserved = 0;
            if (!ok)                // (else the last ticket's)
                map->valid = 0;
        }
    }
    if (!ok)
        return;

    uint8_t *__restrict__ bits = const_cast<uint8_t *>(fold_map_bits(map));
    int2 *__restrict__ out_uv = const_cast<int2 *>(fold_map_uv(map, num_vis));
    int16_t *__restrict__ out_w = const_cast<int16_t *>(fold_map_w(map, num_vis, H));
    const int64_t span_start = (int64_t) blockIdx.x * tiles_per_span * FOLD_TILE;
    int64_t span_end = span_start + tiles_per_span * FOLD_TILE;
    span_end = span_end < num_vis ? span_end : num_vis;
    int64_t run_base = offset;      // output index of the next tile's first head
    int parity = 0;
    for (int64_t tile = span_start; tile < span_end; tile += FOLD_TILE, parity ^= 1) {
        const int64_t i0 = tile + (int64_t) threadIdx.x * FOLD_RECORDS;
        fold_keys keys;
        unsigned heads = 0;
        if (i0 < num_vis) {
            fold_load_keys(uv, w_plane, i0, num_vis, span_start, keys);
            heads = fold_heads(keys, i0, num_vis, span_start);
            bits[i0 / FOLD_RECORDS] = (uint8_t) heads;
        }
        // heads before this thread in its tile: a scan over the wave, the waves' totals through LDS
        const int cnt = __builtin_popcount(heads);
        int inc = cnt;
#pragma unroll
        for (int d = 1; d < WAVE; d *= 2) {
            const int o = __shfl_up(inc, d, WAVE);
            if (lane >= d)
                inc += o;
        }
        if (lane == WAVE - 1)
            s_cnt[parity][wave] = inc;
        __syncthreads();        // (one per tile: s_cnt alternates between two copies)
        int prefix = 0, whole = 0;
#pragma unroll
        for (int w = 0; w < FOLD_WAVES; w++) {
            prefix += w < wave ? s_cnt[parity][w] : 0;
            whole += s_cnt[parity][w];
        }
        int64_t r = run_base + prefix + inc - cnt;
#pragma unroll
        for (int j = 0; j < FOLD_RECORDS; j++) {
            if ((heads >> j) & 1u) {
                if (r < heads_room) {
                    out_uv[r] = keys.uv[j];
                    out_w[r] = (int16_t) keys.wp[j];
                }
                r++;
            }
        }
        run_base += whole;
    }
    if (threadIdx.x == 0) {
        const int64_t mine = run_base - offset;
        const unsigned add = 1u + (mine != (int64_t) plan->counts[blockIdx.x] ? 0x10000u : 0u);
        const unsigned now = atomicAdd(&map->ticket[0], add) + add;
        if ((now & 0xffffu) == (unsigned) spans)
            map->valid = (now >> 16) == 0 ? 1u : 0u;
    }
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

} // namespace

size_t kimg_fold_workspace_bytes(int P, int64_t capacity)
{
    return fold_carve(P, capacity, nullptr).total;
}

int kimg_fold_launch(const int16_t *uv, const int16_t *w_plane, const float2 *vis, int64_t num_vis,
                     int P, int64_t capacity, void *workspace, hipStream_t stream,
                     const kimg_fold_plan_data *plan_data, const kimg_fold_map_data *map)
{
    if (capacity < 0)
        capacity = 0;
    const fold_ws ws = fold_carve(P, capacity, workspace);
    const fold_plan plan = fold_plan_of(num_vis, P);
    if (map != nullptr) {
        // one launch: the samples in, the sums out
        kimg_for_pols(P, [&](auto p) {
            fold_compact_kernel<decltype(p)::value, false, true>
                <<<plan.spans, FOLD_THREADS, 0, stream>>>(
                uv, w_plane, vis, num_vis, plan.tiles_per_span, plan.spans, map->counts, capacity,
                ws.header, ws.uv, ws.w_plane, ws.vis, nullptr, nullptr, map); });
        return kimg_launch_status();
    }
    if (plan_data != nullptr) {
        // the workspace's counts are free for the spans' own counts
        KIMG_HIP(hipMemsetAsync(ws.header->ticket, 0, sizeof(ws.header->ticket), stream));
        kimg_for_pols(P, [&](auto p) {
            fold_compact_kernel<decltype(p)::value, true, false>
                <<<plan.spans, FOLD_THREADS, 0, stream>>>(
                uv, w_plane, vis, num_vis, plan.tiles_per_span, plan.spans, plan_data->counts,
                capacity, ws.header, ws.uv, ws.w_plane, ws.vis, plan_data, ws.counts, nullptr); });
        return kimg_launch_status();
    }
    fold_count_kernel<<<plan.spans, FOLD_THREADS, 0, stream>>>(uv, w_plane, num_vis,
                                                               plan.tiles_per_span, ws.counts);
    kimg_for_pols(P, [&](auto p) {
        fold_compact_kernel<decltype(p)::value, false, false>
            <<<plan.spans, FOLD_THREADS, 0, stream>>>(
            uv, w_plane, vis, num_vis, plan.tiles_per_span, plan.spans, ws.counts, capacity,
            ws.header, ws.uv, ws.w_plane, ws.vis, nullptr, nullptr, nullptr); });
    return kimg_launch_status();
}

extern "C" size_t kimg_fold_map_bytes(int64_t num_vis, int num_polarizations, int64_t heads)
{
    if (num_vis < 1 || num_polarizations < 1 || num_polarizations > 4 || heads < 0)
        return 0;
    return fold_map_bytes(num_vis, heads);
}

extern "C" int kimg_fold_map(const int16_t *uv, const int16_t *w_plane, int64_t num_vis,
                             int num_polarizations, const void *plan, void *map,
                             size_t map_bytes, void *stream)
{
    KIMG_CHECK_ARG(uv && w_plane && plan && map && num_vis >= 1);
    if (num_polarizations < 1 || num_polarizations > 4)
        return KIMG_EUNSUPPORTED;
    KIMG_CHECK_ARG(aligned16(uv) && aligned16(w_plane) && aligned16(plan) && aligned16(map));
    if (map_bytes < fold_map_bytes(num_vis, 0))
        return KIMG_EWORKSPACE;
    // the records the buffer has room for: whole eights of 10 bytes each
    const int64_t heads_room = (int64_t) ((map_bytes - fold_map_bytes(num_vis, 0)) / 80) * 8;
    kimg_fold_map_data *data = static_cast<kimg_fold_map_data *>(map);
    const fold_plan layout = fold_plan_of(num_vis, num_polarizations);
    hipStream_t s = (hipStream_t) stream;
    KIMG_HIP(hipMemsetAsync(data->ticket, 0, sizeof(data->ticket), s));
    fold_map_kernel<<<layout.spans, FOLD_THREADS, 0, s>>>(
        uv, w_plane, num_vis, layout.tiles_per_span, layout.spans,
        static_cast<const kimg_fold_plan_data *>(plan), heads_room, data);
    return kimg_launch_status();
}

extern "C" size_t kimg_fold_plan_bytes(void) { return sizeof(kimg_fold_plan_data); }

extern "C" int kimg_fold_plan(const int16_t *uv, const int16_t *w_plane, int64_t num_vis,
                              int num_polarizations, void *plan, void *stream)
{
    KIMG_CHECK_ARG(uv && w_plane && plan && num_vis >= 1);
    if (num_polarizations < 1 || num_polarizations > 4)
        return KIMG_EUNSUPPORTED;
    KIMG_CHECK_ARG(aligned16(uv) && aligned16(w_plane) && aligned16(plan));
    kimg_fold_plan_data *data = static_cast<kimg_fold_plan_data *>(plan);
    const fold_plan layout = fold_plan_of(num_vis, num_polarizations);
    hipStream_t s = (hipStream_t) stream;
    fold_count_kernel<<<layout.spans, FOLD_THREADS, 0, s>>>(uv, w_plane, num_vis,
                                                            layout.tiles_per_span, data->counts);
    fold_plan_finish_kernel<<<1, FOLD_THREADS, 0, s>>>(data, num_vis, layout.tiles_per_span,
                                                       layout.spans);
    return kimg_launch_status();
}

extern "C" size_t kimg_fold_runs_workspace_bytes(int num_polarizations, int64_t capacity)
{
    if (num_polarizations < 1 || num_polarizations > 4 || capacity < 0)
        return 0;
    return kimg_fold_workspace_bytes(num_polarizations, capacity);
}

static int fold_runs_any(const int16_t *uv, const int16_t *w_plane, const void *vis,
                         int64_t num_vis, int num_polarizations, int64_t capacity, void *workspace,
                         size_t workspace_bytes, void *stream, const void *plan, const void *map)
{
    KIMG_CHECK_ARG(uv && w_plane && vis && workspace && num_vis >= 1 && capacity >= 0);
    if (num_polarizations < 1 || num_polarizations > 4)
        return KIMG_EUNSUPPORTED;
    KIMG_CHECK_ARG(aligned16(uv) && aligned16(w_plane) && aligned16(vis) && aligned16(workspace)
                   && aligned16(plan) && aligned16(map));
    if (workspace_bytes < kimg_fold_workspace_bytes(num_polarizations, capacity))
        return KIMG_EWORKSPACE;
    return kimg_fold_launch(uv, w_plane, static_cast<const float2 *>(vis), num_vis,
                            num_polarizations, capacity, workspace, (hipStream_t) stream,
                            static_cast<const kimg_fold_plan_data *>(plan),
                            static_cast<const kimg_fold_map_data *>(map));
}

extern "C" int kimg_fold_runs_planned(const int16_t *uv, const int16_t *w_plane, const void *vis,
                                      int64_t num_vis, int num_polarizations, int64_t capacity,
                                      void *workspace, size_t workspace_bytes, void *stream,
                                      const void *fold_plan)
{
    return fold_runs_any(uv, w_plane, vis, num_vis, num_polarizations, capacity, workspace,
                         workspace_bytes, stream, fold_plan, nullptr);
}

extern "C" int kimg_fold_runs_mapped(const int16_t *uv, const int16_t *w_plane, const void *vis,
                                     int64_t num_vis, int num_polarizations, int64_t capacity,
                                     void *workspace, size_t workspace_bytes, void *stream,
                                     const void *fold_map)
{
    return fold_runs_any(uv, w_plane, vis, num_vis, num_polarizations, capacity, workspace,
                         workspace_bytes, stream, nullptr, fold_map);
}

extern "C" int kimg_fold_runs(const int16_t *uv, const int16_t *w_plane, const void *vis,
                              int64_t num_vis, int num_polarizations, int64_t capacity,
                              void *workspace, size_t workspace_bytes, void *stream)
{
    return kimg_fold_runs_planned(uv, w_plane, vis, num_vis, num_polarizations, capacity, workspace,
                                  workspace_bytes, stream, nullptr);
}

// (kimg_preload, api.hip)
KIMG_PRELOAD_THIS_UNIT(fold_count_kernel)
