// Per-source moment maps (include/kimg.h, "Per-source moment maps"): the label cube of cube_link.hip
// and the cube read once into the moment maps of EVERY source inside its own bounding box -- a ragged
// table with one entry per (source, pixel of its box).  katsdpimager_amd/source_maps.py holds the same
// contract as numpy (source_maps_host).
//
// The walk is moments.hip's column walk (kimg_cube_column.h): a thread owns V consecutive elements of
// the plane (V = 4 with 16-byte label and cube loads, or 1) for the whole channel loop.  An entry
// belongs to one (source, pixel), a pixel to one thread: every sum has the loop's ascending channel
// order and nothing crosses threads, so there are no atomics and the maps have the bits of
// kimg_moments on the source's own cube (kimg_moment_math.h is compiled into both units).
//
// Per element a thread keeps ONE source in registers: its label, the entry of this pixel in the state
// table and the running sums.  Only when a voxel carries another source's label does the thread store
// the sums to the state table and load the new source's entry, so that a source met again later at the
// same pixel goes on with its own sequential sum; voxels without a label change nothing.  The state
// table is zeroed ahead of the launch, and kimg_source_maps_finish turns it into the maps, a thread per
// entry.
#include "kimg_cube_labels.h"
#include "kimg_moment_math.h"

namespace {

constexpr int SM_THREADS = COL_THREADS;
constexpr int SM_UNROLL = 4;                    // channels whose loads are in flight together
constexpr int SM_ALL = KIMG_MOMENT_0 | KIMG_MOMENT_1 | KIMG_MOMENT_2 | KIMG_MOMENT_8 | KIMG_MOMENT_9
                       | KIMG_MOMENT_COUNT;
constexpr int64_t SM_MAX_TOTAL = (int64_t) INT32_MAX - 1;
constexpr size_t SM_STATE_BYTES = 3 * sizeof(double) + sizeof(float) + 2 * sizeof(int32_t);

using sm_row = kimg_source_map_row;

// The state table inside the workspace: an array per field, `total` entries each
struct sm_state {
    double *S0, *S1, *S2;
    float *peak;
    int32_t *n, *pc;
};

sm_state sm_carve(void *workspace, int64_t total)
{
    sm_state t;
    t.S0 = static_cast<double *>(workspace);
    t.S1 = t.S0 + total;
    t.S2 = t.S1 + total;
    t.peak = reinterpret_cast<float *>(t.S2 + total);
    t.n = reinterpret_cast<int32_t *>(t.peak + total);
    t.pc = t.n + total;
    return t;
}

struct sm_shape {
    int64_t label_pitch, cube_pitch;
    int64_t groups;                 // threads with work
    int64_t base;                   // the plane element of thread 0's first one
    int64_t total;
    int C, H, W, N;
};

// What a thread keeps of one element's current source
struct sm_elem {
    mm_acc acc;
    int32_t label;                  // 0: none yet
    int32_t entry;                  // of this pixel in the source's box; -1: its row leaves the pixel out
    int32_t c0, c1;
    double x_ref;
};

// Plain stores and loads, no atomics: the entry is this pixel's in this source's box, and the pixel is
// this thread's alone for the whole launch -- no other thread reads or writes the entry, and the
// thread's own later load of it follows its store in program order.
__device__ inline void sm_store(const sm_state &t, const sm_elem &s)
{
    if (s.entry < 0)
        return;
    t.S0[s.entry] = s.acc.S0;
    t.S1[s.entry] = s.acc.S1;
    t.S2[s.entry] = s.acc.S2;
    t.peak[s.entry] = s.acc.peak;
    t.n[s.entry] = s.acc.n;
    t.pc[s.entry] = s.acc.pc;
}

// The element (plane index `element`) leaves its source for source `label` (1 .. N).  The rows are the
// caller's device data: nothing read from them becomes an address before it has been checked against
// the box and `total`.
__device__ inline void sm_switch(sm_elem &s, int32_t label, uint32_t element, const sm_shape &g,
                                 const sm_row *__restrict__ rows, const sm_state &t)
{
    sm_store(t, s);
    const sm_row r = rows[label - 1];
    const uint32_t plane = (uint32_t) g.H * (uint32_t) g.W;
    const uint32_t p = element / plane;
    const uint32_t in_plane = element - p * plane;
    const uint32_t y = in_plane / (uint32_t) g.W;
    const uint32_t x = in_plane - y * (uint32_t) g.W;
    const int64_t dy = (int64_t) y - r.y0, dx = (int64_t) x - r.x0;
    const int64_t at = (int64_t) r.offset + dy * r.w + dx;
    const bool inside = (int64_t) p == r.pol && dy >= 0 && dy < r.h && dx >= 0 && dx < r.w
                        && r.offset >= 0 && at < g.total;
    s.label = label;
    s.entry = inside ? (int32_t) at : -1;
    s.c0 = r.c0;
    s.c1 = r.c1;
    s.x_ref = r.x_ref;
    if (inside) {
        s.acc.S0 = t.S0[at];
        s.acc.S1 = t.S1[at];
        s.acc.S2 = t.S2[at];
        s.acc.n = t.n[at];
        s.acc.pc = t.pc[at];
        // (a zeroed entry: nothing has entered yet, the peak starts below everything)
        s.acc.peak = s.acc.n == 0 ? -INFINITY : t.peak[at];
    }
}

// Thread t owns the elements t * V .. t * V + V - 1 of what `labels` and `cube` point at, which are
// the plane elements g.base + t * V ...
template <int V>
__global__ __launch_bounds__(SM_THREADS)
void source_maps_kernel(const int32_t *__restrict__ labels, const float *__restrict__ cube,
                        const sm_shape g, const col_mask filled, const double *__restrict__ x,
                        const sm_row *__restrict__ rows, const sm_state t)
{
    const int64_t id = (int64_t) blockIdx.x * SM_THREADS + threadIdx.x;
    const bool live = id < g.groups;
    // (lanes past the plane run along with clamped addresses, see no label and store nothing)
    const int64_t j = (live ? id : 0) * V;
    const int32_t *lp = labels + j;
    const float *cp = cube + j;
    sm_elem st[V];
#pragma unroll
    for (int e = 0; e < V; e++) {
        st[e].label = 0;
        st[e].entry = -1;
        st[e].c0 = 0;
        st[e].c1 = -1;
        st[e].x_ref = 0.0;
        st[e].acc.S0 = st[e].acc.S1 = st[e].acc.S2 = 0.0;
        st[e].acc.peak = -INFINITY;
        st[e].acc.n = 0;
        st[e].acc.pc = 0;
    }

    for (int cb = 0; cb < g.C; cb += SM_UNROLL) {
        int32_t l[SM_UNROLL][V];
        float v[SM_UNROLL][V];
        bool on[SM_UNROLL];
        const uint64_t have = col_bits_from(filled, cb);
#pragma unroll
        for (int u = 0; u < SM_UNROLL; u++) {
            const int c = cb + u;
            on[u] = c < g.C && ((have >> u) & 1);
#pragma unroll
            for (int e = 0; e < V; e++)
                l[u][e] = 0;
            if (on[u]) {
                if constexpr (V == 4) {
                    const int4 q = *reinterpret_cast<const int4 *>(lp + (int64_t) c * g.label_pitch);
                    l[u][0] = q.x; l[u][1] = q.y; l[u][2] = q.z; l[u][3] = q.w;
                } else {
                    l[u][0] = lp[(int64_t) c * g.label_pitch];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < SM_UNROLL; u++) {
            const int c = cb + u;
            bool any = false;
#pragma unroll
            for (int e = 0; e < V; e++) {
                l[u][e] = live && l[u][e] > 0 && l[u][e] <= g.N ? l[u][e] : 0;
                any |= l[u][e] != 0;
                v[u][e] = col_nan();
            }
            // a wave without a label in this channel reads nothing of the cube
            if (on[u] && __any(any))
                col_load<V>(cp + (int64_t) c * g.cube_pitch, v[u]);
        }
#pragma unroll
        for (int u = 0; u < SM_UNROLL; u++) {
            if (!on[u])
                continue;
            const int c = cb + u;
            const double xc = x[c];
#pragma unroll
            for (int e = 0; e < V; e++) {
                const int32_t label = l[u][e];
                if (label == 0)
                    continue;
                if (label != st[e].label)
                    sm_switch(st[e], label, (uint32_t) (g.base + j + e), g, rows, t);
                if (st[e].entry >= 0 && c >= st[e].c0 && c <= st[e].c1)
                    mm_add<true>(st[e].acc, v[u][e], (double) v[u][e], (double) -INFINITY, xc - st[e].x_ref, c);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < V; e++)
        sm_store(t, st[e]);
}

struct sm_out {
    float *m0, *m1, *m2, *m8, *m9;
    int32_t *count;
};

// One thread per entry: its source is the last row whose offset is not above it (a binary search;
// rows come in ascending offset), if the entry lies inside that row's box at all
__global__ __launch_bounds__(SM_THREADS)
void source_maps_finish_kernel(const sm_row *__restrict__ rows, int N, int64_t total, const sm_state t,
                               const double *__restrict__ x, int C, const sm_out out)
{
    const int64_t i = (int64_t) blockIdx.x * SM_THREADS + threadIdx.x;
    if (i >= total)
        return;
    int lo = 0, hi = N;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (rows[mid].offset <= i)
            lo = mid + 1;
        else
            hi = mid;
    }
    bool owned = false;
    double width = 0.0, x_ref = 0.0;
    if (lo > 0) {
        const sm_row r = rows[lo - 1];
        owned = r.offset >= 0 && r.h > 0 && r.w > 0 && i - r.offset < (int64_t) r.h * r.w;
        width = r.width;
        x_ref = r.x_ref;
    }
    mm_acc a;
    a.S0 = t.S0[i];
    a.S1 = t.S1[i];
    a.S2 = t.S2[i];
    a.peak = t.peak[i];
    a.n = owned ? t.n[i] : 0;
    a.pc = min(max(t.pc[i], 0), C - 1);
    const mm_values v = mm_finish<true>(a, width, x_ref);
    if (out.m0) out.m0[i] = v.m0;
    if (out.m1) out.m1[i] = v.m1;
    if (out.m2) out.m2[i] = v.m2;
    if (out.m8) out.m8[i] = v.m8;
    if (out.m9) out.m9[i] = v.any ? (float) x[a.pc] : col_nan();
    if (out.count) out.count[i] = a.n;
}

template <int V>
void sm_launch(const int32_t *labels, const float *cube, sm_shape g, int64_t base, int64_t groups,
               const col_mask &filled, const double *x, const sm_row *rows, const sm_state &t, hipStream_t s)
{
    g.base = base;
    g.groups = groups;
    source_maps_kernel<V><<<col_blocks(groups), SM_THREADS, 0, s>>>(labels + base, cube + base, g, filled, x,
                                                                    rows, t);
}

}  // namespace

extern "C" size_t kimg_cube_source_maps_workspace_bytes(int64_t total)
{
    if (total <= 0 || total > SM_MAX_TOTAL)
        return 0;
    return (size_t) total * SM_STATE_BYTES;
}

extern "C" int kimg_cube_source_maps(const int32_t *labels, int64_t label_pitch, const float *cube,
                                     int64_t channel_pitch, int num_channels, int num_polarizations,
                                     int height, int width, const uint8_t *filled_host, const double *x,
                                     int num_sources, const kimg_source_map_row *rows, int64_t total,
                                     void *workspace, size_t workspace_bytes, void *stream)
{
    KIMG_CHECK_ARG(labels && cube && filled_host && x && rows && workspace);
    KIMG_CHECK_ARG(lk_aligned(labels, 4) && lk_aligned(cube, 4) && lk_aligned(x, 8) && lk_aligned(rows, 8)
                   && lk_aligned(workspace, 8));
    KIMG_CHECK_ARG(num_channels >= 1 && num_polarizations >= 1 && height >= 1 && width >= 1);
    KIMG_CHECK_ARG(num_sources >= 0 && total >= 0);
    const int64_t PH = (int64_t) num_polarizations * height;
    if (PH > INT32_MAX)
        return KIMG_EUNSUPPORTED;
    const int64_t M = PH * width;
    KIMG_CHECK_ARG(label_pitch >= M && channel_pitch >= M);
    if (!lk_fits(num_channels, M) || total > SM_MAX_TOTAL)
        return KIMG_EUNSUPPORTED;
    if (workspace_bytes < (size_t) total * SM_STATE_BYTES)
        return KIMG_EWORKSPACE;
    if (num_sources == 0 || total == 0)
        return 0;
    hipStream_t s = (hipStream_t) stream;
    KIMG_HIP(hipMemsetAsync(workspace, 0, (size_t) total * SM_STATE_BYTES, s));
    sm_shape g = {};
    g.label_pitch = label_pitch;
    g.cube_pitch = channel_pitch;
    g.total = total;
    g.C = num_channels;
    g.H = height;
    g.W = width;
    g.N = num_sources;
    const col_mask filled = lk_filled_mask(filled_host, num_channels);
    const sm_state t = sm_carve(workspace, total);
    // the form (kimg_cube_column.h): four elements per thread where every address a thread forms is
    // 16-byte aligned, one element per thread for the tail and for everything else
    const uintptr_t alignment = (uintptr_t) labels | ((uintptr_t) label_pitch * sizeof(int32_t))
                                | (uintptr_t) cube | ((uintptr_t) channel_pitch * sizeof(float));
    const int64_t done = col_vector_elements(alignment, M);
    if (done)
        sm_launch<4>(labels, cube, g, 0, done / 4, filled, x, rows, t, s);
    if (done < M)
        sm_launch<1>(labels, cube, g, done, M - done, filled, x, rows, t, s);
    return kimg_launch_status();
}

extern "C" int kimg_source_maps_finish(int num_sources, const kimg_source_map_row *rows, int64_t total,
                                       const void *workspace, size_t workspace_bytes, const double *x,
                                       int num_channels, int outputs, float *moment0, float *moment1,
                                       float *moment2, float *moment8, float *moment9, int32_t *count,
                                       void *stream)
{
    KIMG_CHECK_ARG(rows && workspace && x);
    KIMG_CHECK_ARG(lk_aligned(rows, 8) && lk_aligned(workspace, 8) && lk_aligned(x, 8));
    KIMG_CHECK_ARG(num_sources >= 0 && total >= 0 && num_channels >= 1);
    KIMG_CHECK_ARG(outputs != 0 && (outputs & ~SM_ALL) == 0);
    sm_out out;
    out.m0 = (outputs & KIMG_MOMENT_0) ? moment0 : nullptr;
    out.m1 = (outputs & KIMG_MOMENT_1) ? moment1 : nullptr;
    out.m2 = (outputs & KIMG_MOMENT_2) ? moment2 : nullptr;
    out.m8 = (outputs & KIMG_MOMENT_8) ? moment8 : nullptr;
    out.m9 = (outputs & KIMG_MOMENT_9) ? moment9 : nullptr;
    out.count = (outputs & KIMG_MOMENT_COUNT) ? count : nullptr;
    const void *ptrs[6] = {out.m0, out.m1, out.m2, out.m8, out.m9, out.count};
    const int bits[6] = {KIMG_MOMENT_0, KIMG_MOMENT_1, KIMG_MOMENT_2, KIMG_MOMENT_8, KIMG_MOMENT_9,
                         KIMG_MOMENT_COUNT};
    for (int k = 0; k < 6; k++)
        if (outputs & bits[k])
            KIMG_CHECK_ARG(ptrs[k] && lk_aligned(ptrs[k], 4));
    if (num_channels > COL_MAX_CHANNELS || total > SM_MAX_TOTAL)
        return KIMG_EUNSUPPORTED;
    if (workspace_bytes < (size_t) total * SM_STATE_BYTES)
        return KIMG_EWORKSPACE;
    if (num_sources == 0 || total == 0)
        return 0;
    // (the kernel only reads the state)
    const sm_state t = sm_carve(const_cast<void *>(workspace), total);
    source_maps_finish_kernel<<<col_blocks(total), SM_THREADS, 0, (hipStream_t) stream>>>(
        rows, num_sources, total, t, x, num_channels, out);
    return kimg_launch_status();
}

KIMG_PRELOAD_THIS_UNIT(source_maps_finish_kernel)
