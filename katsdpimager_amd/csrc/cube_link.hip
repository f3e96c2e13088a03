// Source linking (include/kimg.h, "Source linking"): the detection mask [C][M] of cube_detect.hip linked
// into sources -- a label cube int32 [C][M] -- and a catalogue measured from the labels and the cube,
// filtered by size and handed back as a mask.  katsdpimager_amd/link.py holds the same contracts as
// numpy (link_host, measure_host, filter_host, label_mask_host).
//
// The dense launches.  A workgroup of 256 threads owns LK_CHUNK = 1024 consecutive elements of ONE
// channel's plane, a thread four consecutive ones; workgroup b = c * blocks_per_channel + i, so that
// workgroups and, inside one, threads and their elements ascend in the dense index d = c * M + m.  A
// thread whose four elements lie inside the plane takes them with one access where the array's base
// and pitch allow it (mask: 4 bytes, labels: 16 bytes); the last thread of a plane and every thread of
// an array that is not aligned go element by element.  Labels are stored four at a time only by the
// launch that writes the whole label cube (init) and bytes only by kimg_cube_label_mask, which writes
// the whole mask; every other launch stores single labels, under the voxel's own condition.
//
// Linking is a lock-free union-find in the label cube itself: L[d] = d + 1 for a set voxel, and a
// union hangs the larger root under the smaller one with atomicMin, so labels only ever decrease, a
// chain of labels always ends in a root (L[d] == d + 1), and nothing waits for another workgroup.
// Inside the merge launch every read of L is a relaxed agent-scope atomic load: a value read may be
// old, but it was once true, and an old parent still leads to the root.
//
// The launch geometry, the label load, the filled bits and the host's range checks are
// kimg_cube_labels.h's, shared with cube_sources.hip.
#include "kimg_cube_labels.h"

namespace {

constexpr int LK_SCAN_THREADS = 1024;

// What every dense launch knows of the cubes
struct lk_shape {
    int64_t M, blocks_per_channel, mask_pitch, label_pitch;
    int C, P, H, W;
    int mask_wide, label_wide;      // one access for a thread's four mask bytes / four labels
};

// The workgroup's channel and the thread's first element and number of elements (<= 0: none)
__device__ inline void lk_place(const lk_shape &g, int &c, int64_t &j, int &n)
{
    c = (int) (blockIdx.x / g.blocks_per_channel);
    const int64_t i = blockIdx.x - c * g.blocks_per_channel;
    j = (i * LK_THREADS + threadIdx.x) * LK_V;
    n = (int) min((int64_t) LK_V, g.M - j);
}

// The mask bytes of the thread's elements, byte e in bits 8 e .. 8 e + 7; 0 beyond n
__device__ inline uint32_t lk_mask_load(const uint8_t *p, int n, int wide)
{
    if (wide && n == LK_V)
        return *reinterpret_cast<const uint32_t *>(p);
    uint32_t t = 0;
    for (int e = 0; e < n; e++)
        t |= (uint32_t) p[e] << (8 * e);
    return t;
}

// Where the label of dense index d lies
__device__ inline int32_t *lk_at(int32_t *labels, const lk_shape &g, uint32_t d)
{
    if (g.label_pitch == g.M)
        return labels + d;
    const uint32_t c = d / (uint32_t) g.M;
    return labels + (int64_t) c * g.label_pitch + (d - c * (uint32_t) g.M);
}

__device__ inline int32_t lk_read(const int32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of the tree that label a (= dense index + 1) is in.  L[d] <= d + 1 always: it ends.
__device__ inline int32_t lk_find(int32_t *labels, const lk_shape &g, int32_t a)
{
    for (;;) {
        const int32_t up = lk_read(lk_at(labels, g, (uint32_t) a - 1));
        if (up == a)
            return a;
        a = up;
    }
}

__device__ inline void lk_unite(int32_t *labels, const lk_shape &g, int32_t a, int32_t b)
{
    for (;;) {
        a = lk_find(labels, g, a);
        b = lk_find(labels, g, b);
        if (a == b)
            return;
        const int32_t big = max(a, b), small = min(a, b);
        const int32_t old = atomicMin(lk_at(labels, g, (uint32_t) big - 1), small);
        if (old == big)
            return;
        // `big` was no root any more: what it hangs under has to meet `small` instead
        a = old;
        b = small;
    }
}

// Exclusive prefix of k over the workgroup's threads in thread order, and the total; `lds` holds one
// int per wave; two uses must be separated by a barrier
__device__ inline int lk_block_scan(int k, int *lds, int &total)
{
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE, waves = blockDim.x / WAVE;
    int inclusive = k;
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const int t = __shfl_up(inclusive, off, WAVE);
        if (lane >= off)
            inclusive += t;
    }
    if (lane == WAVE - 1)
        lds[wave] = inclusive;
    __syncthreads();
    int before = 0;
    total = 0;
    for (int w = 0; w < waves; w++) {
        const int t = lds[w];
        before += w < wave ? t : 0;
        total += t;
    }
    return before + inclusive - k;
}

// ---- link -------------------------------------------------------------------------------------------

__global__ __launch_bounds__(LK_THREADS)
void lk_init_kernel(const uint8_t *__restrict__ mask, int32_t *__restrict__ labels, const lk_shape g,
                    const col_mask filled)
{
    int c, n;
    int64_t j;
    lk_place(g, c, j, n);
    if (n <= 0)
        return;
    const uint32_t t = lk_filled(filled, c) ? lk_mask_load(mask + c * g.mask_pitch + j, n, g.mask_wide) : 0;
    const int32_t d1 = (int32_t) (c * g.M + j) + 1;
    int32_t v[LK_V];
#pragma unroll
    for (int e = 0; e < LK_V; e++)
        v[e] = ((t >> (8 * e)) & 0xff) ? d1 + e : 0;
    int32_t *to = labels + c * g.label_pitch + j;
    if (g.label_wide && n == LK_V) {
        *reinterpret_cast<int4 *>(to) = make_int4(v[0], v[1], v[2], v[3]);
    } else {
        for (int e = 0; e < n; e++)
            to[e] = v[e];
    }
}

// Every set voxel unites itself with its set neighbours of smaller dense index: the channels
// c - reach_z .. c - 1 with every (dy, dx) of the disc, and in its own channel the rows above and the
// pixels to the left in its own row.  radius = floor(sqrt(reach_xy_sq))
__global__ __launch_bounds__(LK_THREADS)
void lk_merge_kernel(const uint8_t *__restrict__ mask, int32_t *labels, const lk_shape g,
                     const col_mask filled, int reach_xy_sq, int radius, int reach_z)
{
    int c, n;
    int64_t j;
    lk_place(g, c, j, n);
    if (n <= 0 || !lk_filled(filled, c))
        return;
    const uint32_t t = lk_mask_load(mask + c * g.mask_pitch + j, n, g.mask_wide);
    if (!t)
        return;
    const uint32_t plane = (uint32_t) g.H * (uint32_t) g.W;
    for (int e = 0; e < n; e++) {
        if (!((t >> (8 * e)) & 0xff))
            continue;
        const uint32_t m = (uint32_t) (j + e);
        const uint32_t p = m / plane, r = m - p * plane;
        const int y = (int) (r / (uint32_t) g.W), x = (int) (r - (uint32_t) y * g.W);
        const int32_t own = (int32_t) (c * g.M + m) + 1;
        for (int dz = -min(reach_z, c); dz <= 0; dz++) {
            const int cc = c + dz;
            if (!lk_filled(filled, cc))
                continue;
            const uint8_t *row0 = mask + cc * g.mask_pitch + (int64_t) p * plane;
            const int dy_stop = dz ? radius : 0;
            for (int dy = -radius; dy <= dy_stop; dy++) {
                const int yy = y + dy;
                if (yy < 0 || yy >= g.H)
                    continue;
                const int dx_stop = (dz || dy) ? radius : -1;
                for (int dx = -radius; dx <= dx_stop; dx++) {
                    const int xx = x + dx;
                    if (xx < 0 || xx >= g.W || dx * dx + dy * dy > reach_xy_sq)
                        continue;
                    const int64_t mm = (int64_t) p * plane + (int64_t) yy * g.W + xx;
                    if (row0[(int64_t) yy * g.W + xx])
                        lk_unite(labels, g, own, (int32_t) (cc * g.M + mm) + 1);
                }
            }
        }
    }
}

// L[d] = root, and the workgroup's number of roots
__global__ __launch_bounds__(LK_THREADS)
void lk_flatten_kernel(const uint8_t *__restrict__ mask, int32_t *labels, const lk_shape g,
                       const col_mask filled, int32_t *__restrict__ block_roots)
{
    __shared__ int lds[LK_THREADS / WAVE];
    int c, n;
    int64_t j;
    lk_place(g, c, j, n);
    int roots = 0;
    if (n > 0 && lk_filled(filled, c)) {
        const uint32_t t = lk_mask_load(mask + c * g.mask_pitch + j, n, g.mask_wide);
        int32_t *mine = labels + c * g.label_pitch + j;
        const int32_t d1 = (int32_t) (c * g.M + j) + 1;
        for (int e = 0; t && e < n; e++) {
            if (!((t >> (8 * e)) & 0xff))
                continue;
            const int32_t up = lk_read(mine + e);
            const int32_t root = up == d1 + e ? up : lk_find(labels, g, up);
            if (root != up)
                mine[e] = root;
            roots += root == d1 + e;
        }
    }
    int total;
    lk_block_scan(roots, lds, total);
    if (threadIdx.x == 0)
        block_roots[blockIdx.x] = total;
}

// block_roots [blocks] becomes its exclusive prefix, in place; *total = their sum.  One workgroup: a
// thread sums a run of consecutive entries, the runs are scanned, the thread writes its run back.
__global__ __launch_bounds__(LK_SCAN_THREADS)
void lk_scan_kernel(int32_t *block_roots, int64_t blocks, int32_t *total_out)
{
    __shared__ int lds[LK_SCAN_THREADS / WAVE];
    const int64_t per = (blocks + LK_SCAN_THREADS - 1) / LK_SCAN_THREADS;
    const int64_t from = min(blocks, per * threadIdx.x), to = min(blocks, from + per);
    int sum = 0;
    for (int64_t i = from; i < to; i++)
        sum += block_roots[i];
    int total;
    int before = lk_block_scan(sum, lds, total);
    for (int64_t i = from; i < to; i++) {
        const int t = block_roots[i];
        block_roots[i] = before;
        before += t;
    }
    if (threadIdx.x == 0)
        *total_out = total;
}

// Roots get the negated number of their source: its rank among the roots in ascending dense index, + 1
__global__ __launch_bounds__(LK_THREADS)
void lk_number_kernel(const uint8_t *__restrict__ mask, int32_t *labels, const lk_shape g,
                      const col_mask filled, const int32_t *__restrict__ block_roots)
{
    __shared__ int lds[LK_THREADS / WAVE];
    int c, n;
    int64_t j;
    lk_place(g, c, j, n);
    uint32_t is_root = 0;
    int32_t *mine = labels + c * g.label_pitch + j;
    if (n > 0 && lk_filled(filled, c)) {
        const uint32_t t = lk_mask_load(mask + c * g.mask_pitch + j, n, g.mask_wide);
        const int32_t d1 = (int32_t) (c * g.M + j) + 1;
        for (int e = 0; t && e < n; e++)
            if (((t >> (8 * e)) & 0xff) && mine[e] == d1 + e)
                is_root |= 1u << e;
    }
    int total;
    int rank = lk_block_scan(__popc(is_root), lds, total) + block_roots[blockIdx.x];
    for (int e = 0; is_root && e < LK_V; e++)
        if ((is_root >> e) & 1)
            mine[e] = -(++rank);
}

// Every set voxel gets the number of its source: a root (negative) its own, every other voxel (which
// points at its root since the flatten launch) the root's -- negative or, where the root's own thread
// has come by already, positive: its magnitude either way
__global__ __launch_bounds__(LK_THREADS)
void lk_relabel_kernel(const uint8_t *__restrict__ mask, int32_t *labels, const lk_shape g,
                       const col_mask filled)
{
    int c, n;
    int64_t j;
    lk_place(g, c, j, n);
    if (n <= 0 || !lk_filled(filled, c))
        return;
    const uint32_t t = lk_mask_load(mask + c * g.mask_pitch + j, n, g.mask_wide);
    int32_t *mine = labels + c * g.label_pitch + j;
    for (int e = 0; t && e < n; e++) {
        if (!((t >> (8 * e)) & 0xff))
            continue;
        const int32_t v = lk_read(mine + e);
        const int32_t number = v < 0 ? -v : abs(lk_read(lk_at(labels, g, (uint32_t) v - 1)));
        __hip_atomic_store(mine + e, number, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- measure ----------------------------------------------------------------------------------------

// kimg_catalogue by value, plus the keys in its work area
struct lk_rows {
    kimg_catalogue t;
    int capacity;
};

__device__ inline unsigned long long *lk_peak_keys(const lk_rows &r) { return (unsigned long long *) r.t.work; }
__device__ inline unsigned long long *lk_trough_keys(const lk_rows &r)
{
    return (unsigned long long *) r.t.work + r.capacity;
}
__device__ inline int32_t *lk_remap(const lk_rows &r) { return (int32_t *) ((unsigned long long *) r.t.work + 2 * (size_t) r.capacity); }

// kimg_cube_stats' order of float32 values as an unsigned integer: -0 below +0
__device__ inline uint32_t lk_value_key(float f)
{
    const uint32_t bits = __float_as_uint(f);
    return bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u);
}

__device__ inline float lk_key_value(uint32_t key)
{
    return __uint_as_float(key ^ ((key >> 31) ? 0x80000000u : 0xffffffffu));
}

__global__ __launch_bounds__(LK_THREADS)
void lk_rows_init_kernel(const lk_rows r, const int32_t *__restrict__ counts)
{
    const int s = blockIdx.x * LK_THREADS + threadIdx.x;
    if (s >= min(counts[0], r.capacity))
        return;
    r.t.first[s] = INT32_MAX;
    r.t.voxels[s] = 0;
    r.t.finite[s] = 0;
    r.t.c0[s] = INT32_MAX; r.t.c1[s] = -1;
    r.t.y0[s] = INT32_MAX; r.t.y1[s] = -1;
    r.t.x0[s] = INT32_MAX; r.t.x1[s] = -1;
    r.t.sum[s] = 0.0; r.t.sum_c[s] = 0.0; r.t.sum_y[s] = 0.0; r.t.sum_x[s] = 0.0;
    lk_peak_keys(r)[s] = 0;
    lk_trough_keys(r)[s] = 0;
}

// The run of equal labels that a thread's element is in, along the channel axis
struct lk_run {
    int32_t label, c0, c1, voxels, finite;
    double s, sc, sy, sx;
    unsigned long long peak, trough;
};

__device__ inline void lk_flush(const lk_run &run, const lk_rows &r, int32_t first, int y, int x)
{
    const int s = run.label - 1;
    if (s >= r.capacity)
        return;
    atomicAdd(r.t.voxels + s, run.voxels);
    atomicMin(r.t.first + s, first);
    atomicMin(r.t.c0 + s, run.c0);
    atomicMax(r.t.c1 + s, run.c1);
    atomicMin(r.t.y0 + s, y);
    atomicMax(r.t.y1 + s, y);
    atomicMin(r.t.x0 + s, x);
    atomicMax(r.t.x1 + s, x);
    if (run.finite) {
        atomicAdd(r.t.finite + s, run.finite);
        atomicMax(lk_peak_keys(r) + s, run.peak);
        atomicMax(lk_trough_keys(r) + s, run.trough);
        atomicAdd(r.t.sum + s, run.s);
        atomicAdd(r.t.sum_c + s, run.sc);
        atomicAdd(r.t.sum_y + s, run.sy);
        atomicAdd(r.t.sum_x + s, run.sx);
    }
}

// A thread owns four consecutive elements of the plane for the whole channel loop
__global__ __launch_bounds__(LK_THREADS)
void lk_measure_kernel(const int32_t *__restrict__ labels, const float *__restrict__ cube,
                       int64_t pitch, int cube_wide, const lk_shape g, const col_mask filled,
                       const lk_rows r)
{
    const int64_t j = ((int64_t) blockIdx.x * LK_THREADS + threadIdx.x) * LK_V;
    const int n = (int) min((int64_t) LK_V, g.M - j);
    if (n <= 0)
        return;
    const uint32_t plane = (uint32_t) g.H * (uint32_t) g.W;
    int y[LK_V], x[LK_V];
    lk_run run[LK_V];
#pragma unroll
    for (int e = 0; e < LK_V; e++) {
        const uint32_t m = (uint32_t) (j + min(e, n - 1));
        const uint32_t rest = m % plane;
        y[e] = (int) (rest / (uint32_t) g.W);
        x[e] = (int) (rest - (uint32_t) y[e] * g.W);
        run[e].label = 0;
    }
    for (int c = 0; c < g.C; c++) {
        int32_t l[LK_V] = {0, 0, 0, 0};
        float f[LK_V] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (lk_filled(filled, c)) {
            lk_label_load(labels + c * g.label_pitch + j, n, g.label_wide, l);
            if (l[0] > 0 || l[1] > 0 || l[2] > 0 || l[3] > 0) {
                const float *from = cube + c * pitch + j;
                if (cube_wide && n == LK_V) {
                    col_load<LK_V>(from, f);
                } else {
                    for (int e = 0; e < n; e++)
                        f[e] = from[e];
                }
            }
        }
#pragma unroll
        for (int e = 0; e < LK_V; e++) {
            const int32_t label = max(l[e], 0);
            if (label != run[e].label) {
                if (run[e].label)
                    lk_flush(run[e], r, (int32_t) (run[e].c0 * g.M + j + e), y[e], x[e]);
                run[e].label = label;
                run[e].c0 = c;
                run[e].voxels = 0;
                run[e].finite = 0;
                run[e].s = 0.0; run[e].sc = 0.0; run[e].sy = 0.0; run[e].sx = 0.0;
                run[e].peak = 0;
                run[e].trough = 0;
            }
            if (label) {
                run[e].c1 = c;
                run[e].voxels++;
                const float v = f[e];
                if ((__float_as_uint(v) & 0x7f800000u) != 0x7f800000u) {
                    const double t = (double) v;
                    run[e].finite++;
                    run[e].s = run[e].s + t;
                    run[e].sc = run[e].sc + t * (double) c;
                    run[e].sy = run[e].sy + t * (double) y[e];
                    run[e].sx = run[e].sx + t * (double) x[e];
                    const uint32_t key = lk_value_key(v);
                    const uint32_t where = ~(uint32_t) (c * g.M + j + e);
                    run[e].peak = max(run[e].peak, ((unsigned long long) key << 32) | where);
                    run[e].trough = max(run[e].trough, ((unsigned long long) ~key << 32) | where);
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < LK_V; e++)
        if (run[e].label)
            lk_flush(run[e], r, (int32_t) (run[e].c0 * g.M + j + e), y[e], x[e]);
}

__global__ __launch_bounds__(LK_THREADS)
void lk_rows_finish_kernel(const lk_rows r, const int32_t *__restrict__ counts)
{
    const int s = blockIdx.x * LK_THREADS + threadIdx.x;
    if (s >= min(counts[0], r.capacity))
        return;
    const unsigned long long peak = lk_peak_keys(r)[s], trough = lk_trough_keys(r)[s];
    const bool any = r.t.finite[s] > 0;
    r.t.peak[s] = any ? lk_key_value((uint32_t) (peak >> 32)) : col_nan();
    r.t.peak_index[s] = any ? (int32_t) ~(uint32_t) peak : -1;
    r.t.trough[s] = any ? lk_key_value(~(uint32_t) (trough >> 32)) : col_nan();
    r.t.trough_index[s] = any ? (int32_t) ~(uint32_t) trough : -1;
}

// ---- filter -----------------------------------------------------------------------------------------

struct lk_row {
    int32_t i[11];
    float f[2];
    double d[4];
};

__device__ inline void lk_row_load(const kimg_catalogue &t, int s, lk_row &w)
{
    w.i[0] = t.first[s]; w.i[1] = t.voxels[s]; w.i[2] = t.finite[s];
    w.i[3] = t.c0[s]; w.i[4] = t.c1[s]; w.i[5] = t.y0[s]; w.i[6] = t.y1[s]; w.i[7] = t.x0[s]; w.i[8] = t.x1[s];
    w.i[9] = t.peak_index[s]; w.i[10] = t.trough_index[s];
    w.f[0] = t.peak[s]; w.f[1] = t.trough[s];
    w.d[0] = t.sum[s]; w.d[1] = t.sum_c[s]; w.d[2] = t.sum_y[s]; w.d[3] = t.sum_x[s];
}

__device__ inline void lk_row_store(const kimg_catalogue &t, int s, const lk_row &w)
{
    t.first[s] = w.i[0]; t.voxels[s] = w.i[1]; t.finite[s] = w.i[2];
    t.c0[s] = w.i[3]; t.c1[s] = w.i[4]; t.y0[s] = w.i[5]; t.y1[s] = w.i[6]; t.x0[s] = w.i[7]; t.x1[s] = w.i[8];
    t.peak_index[s] = w.i[9]; t.trough_index[s] = w.i[10];
    t.peak[s] = w.f[0]; t.trough[s] = w.f[1];
    t.sum[s] = w.d[0]; t.sum_c[s] = w.d[1]; t.sum_y[s] = w.d[2]; t.sum_x[s] = w.d[3];
}

// One workgroup walks the rows in tiles of its size, in ascending order: a tile is read into
// registers, then its kept rows are written to the front.  A row never moves to a higher place, so a
// tile overwrites only rows of its own (already read: the barrier) and of tiles before it.  With more
// sources than rows nothing is changed and counts[1] = counts[0].
__global__ __launch_bounds__(LK_SCAN_THREADS)
void lk_filter_kernel(const lk_rows r, int32_t *counts, int min_voxels, int min_size_xy, int min_size_z)
{
    __shared__ int lds[LK_SCAN_THREADS / WAVE];
    const int rows = counts[0];
    if (rows > r.capacity) {
        if (threadIdx.x == 0)
            counts[1] = rows;
        return;
    }
    int32_t *remap = lk_remap(r);
    int kept = 0;
    for (int base = 0; base < rows; base += LK_SCAN_THREADS) {
        const int s = base + threadIdx.x;
        lk_row w;
        bool keep = false;
        if (s < rows) {
            lk_row_load(r.t, s, w);
            keep = w.i[1] >= min_voxels && w.i[8] - w.i[7] + 1 >= min_size_xy
                   && w.i[6] - w.i[5] + 1 >= min_size_xy && w.i[4] - w.i[3] + 1 >= min_size_z;
        }
        int total;
        const int to = kept + lk_block_scan(keep, lds, total);      // (its barrier: the tile is read)
        if (s < rows)
            remap[s] = keep ? to + 1 : 0;
        if (keep)
            lk_row_store(r.t, to, w);
        kept += total;
        __syncthreads();
    }
    if (threadIdx.x == 0)
        counts[1] = kept;
}

__global__ __launch_bounds__(LK_THREADS)
void lk_renumber_kernel(int32_t *labels, const lk_shape g, const lk_rows r,
                        const int32_t *__restrict__ counts)
{
    int c, n;
    int64_t j;
    lk_place(g, c, j, n);
    if (n <= 0 || counts[0] > r.capacity)
        return;
    const int rows = counts[0];
    const int32_t *remap = lk_remap(r);
    int32_t *mine = labels + c * g.label_pitch + j;
    int32_t l[LK_V];
    lk_label_load(mine, n, g.label_wide, l);
    for (int e = 0; e < n; e++) {
        if (l[e] <= 0)
            continue;
        const int32_t number = l[e] <= rows ? remap[l[e] - 1] : 0;
        if (number != l[e])
            mine[e] = number;
    }
}

// ---- label mask -------------------------------------------------------------------------------------

__global__ __launch_bounds__(LK_THREADS)
void lk_label_mask_kernel(const int32_t *__restrict__ labels, uint8_t *__restrict__ mask,
                          const lk_shape g, int source)
{
    int c, n;
    int64_t j;
    lk_place(g, c, j, n);
    if (n <= 0)
        return;
    int32_t l[LK_V];
    lk_label_load(labels + c * g.label_pitch + j, n, g.label_wide, l);
    uint32_t t = 0;
#pragma unroll
    for (int e = 0; e < LK_V; e++)
        t |= (uint32_t) (source ? l[e] == source : l[e] != 0) << (8 * e);
    uint8_t *to = mask + c * g.mask_pitch + j;
    if (g.mask_wide && n == LK_V) {
        *reinterpret_cast<uint32_t *>(to) = t;
    } else {
        for (int e = 0; e < n; e++)
            to[e] = (uint8_t) (t >> (8 * e));
    }
}

// ---- host -------------------------------------------------------------------------------------------

lk_shape lk_shape_of(int C, int P, int H, int W, int64_t M, const void *mask, int64_t mask_pitch,
                     const void *labels, int64_t label_pitch)
{
    lk_shape g;
    g.M = M;
    g.blocks_per_channel = lk_blocks_per_channel(M);
    g.mask_pitch = mask_pitch;
    g.label_pitch = label_pitch;
    g.C = C; g.P = P; g.H = H; g.W = W;
    g.mask_wide = (((uintptr_t) mask | (uintptr_t) mask_pitch) & 3) == 0;
    g.label_wide = (((uintptr_t) labels | ((uintptr_t) label_pitch * 4)) & 15) == 0;
    return g;
}

unsigned lk_blocks(const lk_shape &g) { return (unsigned) (g.blocks_per_channel * g.C); }

bool lk_catalogue_ok(const kimg_catalogue *t)
{
    if (!t)
        return false;
    const void *four[] = {t->first, t->voxels, t->finite, t->c0, t->c1, t->y0, t->y1, t->x0, t->x1,
                          t->peak, t->peak_index, t->trough, t->trough_index};
    const void *eight[] = {t->sum, t->sum_c, t->sum_y, t->sum_x, t->work};
    for (const void *p : four)
        if (!p || !lk_aligned(p, 4))
            return false;
    for (const void *p : eight)
        if (!p || !lk_aligned(p, 8))
            return false;
    return true;
}

bool lk_plane_ok(int P, int H, int W, int64_t &M)
{
    if (P < 1 || H < 1 || W < 1 || (int64_t) H * W > INT64_MAX / 4 / P)
        return false;
    M = (int64_t) P * H * W;
    return true;
}

}  // namespace

extern "C" size_t kimg_cube_link_scratch_bytes(int num_channels, int64_t plane_elements)
{
    if (num_channels < 1 || plane_elements < 0 || !lk_fits(num_channels, plane_elements))
        return 0;
    return (size_t) (lk_blocks_per_channel(plane_elements) * num_channels + 4) * sizeof(int32_t);
}

extern "C" size_t kimg_cube_catalogue_work_bytes(int capacity)
{
    return capacity < 1 ? 0 : (size_t) capacity * 24;
}

extern "C" int kimg_cube_link(const uint8_t *mask, int64_t mask_pitch, int32_t *labels,
                              int64_t label_pitch, int num_channels, int num_polarizations, int height,
                              int width, const uint8_t *filled_host, int reach_xy_sq, int reach_z,
                              void *scratch, int32_t *counts, void *stream)
{
    KIMG_CHECK_ARG(mask && labels && filled_host && scratch && counts);
    KIMG_CHECK_ARG(num_channels >= 1);
    int64_t M;
    KIMG_CHECK_ARG(lk_plane_ok(num_polarizations, height, width, M));
    KIMG_CHECK_ARG(mask_pitch >= M && label_pitch >= M);
    KIMG_CHECK_ARG(lk_aligned(labels, 4) && lk_aligned(scratch, 4) && lk_aligned(counts, 4));
    KIMG_CHECK_ARG(reach_xy_sq >= 0 && reach_xy_sq <= 9 && reach_z >= 0 && reach_z <= 3);
    if (!lk_fits(num_channels, M))
        return KIMG_EUNSUPPORTED;
    const col_mask filled = lk_filled_mask(filled_host, num_channels);
    const lk_shape g = lk_shape_of(num_channels, num_polarizations, height, width, M, mask, mask_pitch,
                                   labels, label_pitch);
    hipStream_t s = (hipStream_t) stream;
    const unsigned blocks = lk_blocks(g);
    int32_t *block_roots = (int32_t *) scratch;
    int radius = 0;
    while ((radius + 1) * (radius + 1) <= reach_xy_sq)
        radius++;
    lk_init_kernel<<<blocks, LK_THREADS, 0, s>>>(mask, labels, g, filled);
    lk_merge_kernel<<<blocks, LK_THREADS, 0, s>>>(mask, labels, g, filled, reach_xy_sq, radius, reach_z);
    lk_flatten_kernel<<<blocks, LK_THREADS, 0, s>>>(mask, labels, g, filled, block_roots);
    lk_scan_kernel<<<1, LK_SCAN_THREADS, 0, s>>>(block_roots, blocks, counts);
    lk_number_kernel<<<blocks, LK_THREADS, 0, s>>>(mask, labels, g, filled, block_roots);
    lk_relabel_kernel<<<blocks, LK_THREADS, 0, s>>>(mask, labels, g, filled);
    return kimg_launch_status();
}

extern "C" int kimg_cube_measure(const int32_t *labels, int64_t label_pitch, const float *cube,
                                 int64_t channel_pitch, int num_channels, int num_polarizations,
                                 int height, int width, const uint8_t *filled_host,
                                 const kimg_catalogue *catalogue, int capacity, const int32_t *counts,
                                 void *stream)
{
    KIMG_CHECK_ARG(labels && cube && filled_host && counts);
    KIMG_CHECK_ARG(num_channels >= 1);
    int64_t M;
    KIMG_CHECK_ARG(lk_plane_ok(num_polarizations, height, width, M));
    KIMG_CHECK_ARG(label_pitch >= M && channel_pitch >= M);
    KIMG_CHECK_ARG(lk_aligned(labels, 4) && lk_aligned(cube, 4) && lk_aligned(counts, 4));
    KIMG_CHECK_ARG(capacity >= 1 && lk_catalogue_ok(catalogue));
    if (!lk_fits(num_channels, M))
        return KIMG_EUNSUPPORTED;
    const col_mask filled = lk_filled_mask(filled_host, num_channels);
    const lk_shape g = lk_shape_of(num_channels, num_polarizations, height, width, M, nullptr, M, labels,
                                   label_pitch);
    const lk_rows r = {*catalogue, capacity};
    const int cube_wide = (((uintptr_t) cube | ((uintptr_t) channel_pitch * 4)) & 15) == 0;
    hipStream_t s = (hipStream_t) stream;
    const unsigned row_blocks = (unsigned) kimg_divup(capacity, LK_THREADS);
    lk_rows_init_kernel<<<row_blocks, LK_THREADS, 0, s>>>(r, counts);
    lk_measure_kernel<<<(unsigned) g.blocks_per_channel, LK_THREADS, 0, s>>>(
        labels, cube, channel_pitch, cube_wide, g, filled, r);
    lk_rows_finish_kernel<<<row_blocks, LK_THREADS, 0, s>>>(r, counts);
    return kimg_launch_status();
}

extern "C" int kimg_cube_link_filter(int32_t *labels, int64_t label_pitch, int num_channels,
                                     int64_t plane_elements, const kimg_catalogue *catalogue,
                                     int capacity, int min_voxels, int min_size_xy, int min_size_z,
                                     int32_t *counts, void *stream)
{
    KIMG_CHECK_ARG(labels && counts);
    KIMG_CHECK_ARG(num_channels >= 1 && plane_elements >= 0);
    KIMG_CHECK_ARG(label_pitch >= plane_elements);
    KIMG_CHECK_ARG(lk_aligned(labels, 4) && lk_aligned(counts, 4));
    KIMG_CHECK_ARG(capacity >= 1 && lk_catalogue_ok(catalogue));
    KIMG_CHECK_ARG(min_voxels >= 1 && min_size_xy >= 1 && min_size_z >= 1);
    if (!lk_fits(num_channels, plane_elements))
        return KIMG_EUNSUPPORTED;
    const lk_shape g = lk_shape_of(num_channels, 1, 1, 1, plane_elements, nullptr, plane_elements, labels,
                                   label_pitch);
    const lk_rows r = {*catalogue, capacity};
    hipStream_t s = (hipStream_t) stream;
    lk_filter_kernel<<<1, LK_SCAN_THREADS, 0, s>>>(r, counts, min_voxels, min_size_xy, min_size_z);
    if (plane_elements)
        lk_renumber_kernel<<<lk_blocks(g), LK_THREADS, 0, s>>>(labels, g, r, counts);
    return kimg_launch_status();
}

extern "C" int kimg_cube_label_mask(const int32_t *labels, int64_t label_pitch, uint8_t *mask,
                                    int64_t mask_pitch, int num_channels, int64_t plane_elements,
                                    int source, void *stream)
{
    KIMG_CHECK_ARG(labels && mask);
    KIMG_CHECK_ARG(num_channels >= 1 && plane_elements >= 0);
    KIMG_CHECK_ARG(label_pitch >= plane_elements && mask_pitch >= plane_elements);
    KIMG_CHECK_ARG(lk_aligned(labels, 4) && source >= 0);
    if (!lk_fits(num_channels, plane_elements))
        return KIMG_EUNSUPPORTED;
    if (plane_elements == 0)
        return 0;
    const lk_shape g = lk_shape_of(num_channels, 1, 1, 1, plane_elements, mask, mask_pitch, labels,
                                   label_pitch);
    lk_label_mask_kernel<<<lk_blocks(g), LK_THREADS, 0, (hipStream_t) stream>>>(labels, mask, g, source);
    return kimg_launch_status();
}

KIMG_PRELOAD_THIS_UNIT(lk_label_mask_kernel)
