// Tile-binned gridding: the window gridder (grid_mfma.hip) for visibility streams WITHOUT locality.
//
// The window kernel keeps a 32x32 piece of the grid in a wave's accumulators and lives on
// consecutive visibilities landing in (nearly) the same place: true for the baseline-sorted,
// adjacent-merged stream the reference's preprocessor delivers (loader_ms.py:465-467,
// preprocess.cpp:334-397), false for a time-ordered or shuffled stream, where every record
// costs a whole-window flush (8 KB of float atomics) and the kernel degenerates to the atomic rate
// of the per-tap kernel (grid.mako's situation without its bin sort).  This file restores the
// locality on the device:
//   1. key = bin of the footprint origin, bins of (window slack + 1)^2 cells in serpentine row
//      order -- all visibilities of a bin share one window position, neighbouring bins differ by a
//      partial window move;
//   2. stable radix sort of (key, index) pairs (hipCUB / rocPRIM), only the bits the key needs;
//   3. gather uv / w_plane / vis into sorted copies (one pass, 18 + 8 P bytes per visibility);
//   4. the unchanged window kernel over the sorted copies.
// Results equal the direct path's up to the order of float additions.
// kimg_grid_jumps counts the records that would force a window jump, so that callers can choose.
#include "kimg_record_stream.h"
#include "kimg_window_plan.h"

namespace {

struct bin_geometry {
    int half;           // grid_size / 2: u + half is a non-negative cell index
    int bin;            // cells per bin along either axis
    int nbu;            // bins per row
    unsigned last_key;  // key of records outside the grid (sorted to the end; the kernel skips them)
};

__global__ __launch_bounds__(256) void bin_key_kernel(
    const int16_t *__restrict__ uv, int64_t n, bin_geometry g, int grid_size,
    unsigned *__restrict__ keys, unsigned *__restrict__ index)
{
    const int64_t i = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const vis_coord c = load_uv(uv, i);
    const int u = c.u + g.half, v = c.v + g.half;
    unsigned key = g.last_key;
    if ((unsigned) u < (unsigned) grid_size && (unsigned) v < (unsigned) grid_size) {
        const int bv = v / g.bin;
        int bu = u / g.bin;
        if (bv & 1)
            bu = g.nbu - 1 - bu;        // serpentine: the end of a bin row is next to the start of the next
        key = (unsigned) bv * (unsigned) g.nbu + (unsigned) bu;
    }
    keys[i] = key;
    index[i] = (unsigned) i;
}

// The stream in tile order; WEIGHTS: the degridder's (it also needs the statistical weights) ...
template <int P, bool WEIGHTS>
__global__ __launch_bounds__(256) void gather_kernel(
    const unsigned *__restrict__ index, int64_t n, const int2 *__restrict__ uv,
    const int16_t *__restrict__ w_plane, const float *__restrict__ weights,
    const float2 *__restrict__ vis, int2 *__restrict__ uv_out, int16_t *__restrict__ wp_out,
    float *__restrict__ w_out, float2 *__restrict__ vis_out)
{
    const int64_t i = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const int64_t src = index[i];
    copy_record<P, WEIGHTS>(i, src, uv, w_plane, weights, vis, uv_out, wp_out, w_out, vis_out);
}

// ... and the degridder's results back in the caller's order
template <int P>
__global__ __launch_bounds__(256) void scatter_vis_kernel(
    const unsigned *__restrict__ index, int64_t n, const float2 *__restrict__ vis_sorted,
    float2 *__restrict__ vis)
{
    const int64_t i = blockIdx.x * (int64_t) blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const int64_t dst = index[i];
#pragma unroll
    for (int p = 0; p < P; p++)
        vis[dst * P + p] = vis_sorted[i * P + p];
}

__global__ __launch_bounds__(256) void jump_count_kernel(
    const int16_t *__restrict__ uv, int64_t n, int slack, unsigned *__restrict__ count)
{
    unsigned local = 0;
    for (int64_t i = blockIdx.x * (int64_t) blockDim.x + threadIdx.x + 1; i < n;
         i += (int64_t) gridDim.x * blockDim.x) {
        const vis_coord a = load_uv(uv, i - 1), b = load_uv(uv, i);
        const int du = b.u - a.u, dv = b.v - a.v;
        local += (abs(du) > slack || abs(dv) > slack) ? 1u : 0u;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        local += __shfl_xor(local, off, WAVE);
    if ((threadIdx.x & 63) == 0 && local)
        atomicAdd(count, local);
}

struct binned_ws {
    void *table;        // the window kernel's own scratch (padded table copy), first
    index_sort<unsigned> sort;
    int2 *uv;
    int16_t *wp;
    float2 *vis;
    float *weights;     // degridders only
    void *cub;
    size_t table_bytes, cub_bytes, total;
};

// (`workspace` null: the size only)
hipError_t carve(int64_t n, int P, int W, int OV, int K, bool degrid, void *workspace, binned_ws &ws)
{
    ws_carver c(workspace);
    ws.table = c.take<unsigned char>(degrid ? kimg_degrid_mfma_workspace_bytes(P, W, OV, K)
                                            : kimg_grid_mfma_workspace_bytes(P, W, OV, K));
    ws.table_bytes = c.total();
    ws.sort.carve(c, n);
    ws.uv = c.take<int2>((size_t) n);
    ws.wp = c.take<int16_t>((size_t) n);
    ws.vis = c.take<float2>((size_t) n * P);
    ws.weights = degrid ? c.take<float>((size_t) n * P) : nullptr;
    const hipError_t e = ws.sort.temp_bytes(n, ws.cub_bytes);
    ws.cub = c.take<unsigned char>(ws.cub_bytes);
    ws.total = c.total();
    return e;
}

size_t binned_workspace_bytes(int64_t n, int P, int W, int OV, int K, bool degrid)
{
    if (n <= 0 || n >= ((int64_t) 1 << 31)
        || !(degrid ? kimg_degrid_mfma_supported(P, W, OV, K) : kimg_grid_mfma_supported(P, W, OV, K)))
        return 0;
    binned_ws ws;
    if (carve(n, P, W, OV, K, degrid, nullptr, ws) != hipSuccess)
        return 0;
    return ws.total;
}

} // namespace

int kimg_bin_stream(const int16_t *uv, const int16_t *w_plane, const float *weights, const void *vis,
                    int64_t num_vis, int grid_size, int P, int w_planes, int oversample,
                    int kernel_width, void *workspace, size_t workspace_bytes, hipStream_t stream,
                    kimg_binned_stream &out)
{
    if (num_vis >= ((int64_t) 1 << 31))
        return KIMG_EUNSUPPORTED;
    binned_ws ws;
    hipError_t e = carve(num_vis, P, w_planes, oversample, kernel_width, weights != nullptr, workspace, ws);
    if (e != hipSuccess)
        return -(int) e;
    if (workspace == nullptr || workspace_bytes < ws.total)
        return KIMG_EWORKSPACE;
    // keys of the footprint-origin bins, sorted; out.index = the caller's record of sorted place i
    bin_geometry g;
    g.half = grid_size / 2;
    g.bin = window_slack(kernel_width) + 1;
    g.nbu = (grid_size + g.bin - 1) / g.bin;
    const int nbv = g.nbu;
    g.last_key = (unsigned) g.nbu * (unsigned) nbv;
    const int blocks = kimg_divup(num_vis, 256);
    bin_key_kernel<<<blocks, 256, 0, stream>>>(uv, num_vis, g, grid_size, ws.sort.keys[0],
                                               ws.sort.index[0]);
    KIMG_HIP(ws.sort.sort(ws.cub, ws.cub_bytes, num_vis, sort_bits(g.last_key), stream, out.index));
    int rc = kimg_launch_status();
    if (rc)
        return rc;
    out.uv = reinterpret_cast<const int16_t *>(ws.uv);
    out.w_plane = ws.wp;
    out.vis = ws.vis;
    out.weights = ws.weights;
    out.table = ws.table;
    out.table_bytes = ws.table_bytes;
    const int2 *uv2 = reinterpret_cast<const int2 *>(uv);
    const float2 *vis2 = static_cast<const float2 *>(vis);
    kimg_for_pols(P, [&](auto p) {
        if (weights)
            gather_kernel<decltype(p)::value, true><<<blocks, 256, 0, stream>>>(
                out.index, num_vis, uv2, w_plane, weights, vis2, ws.uv, ws.wp, ws.weights, ws.vis);
        else
            gather_kernel<decltype(p)::value, false><<<blocks, 256, 0, stream>>>(
                out.index, num_vis, uv2, w_plane, nullptr, vis2, ws.uv, ws.wp, nullptr, ws.vis); });
    return kimg_launch_status();
}

int kimg_unbin_vis(const kimg_binned_stream &b, void *vis, int64_t num_vis, int P, hipStream_t stream)
{
    kimg_for_pols(P, [&](auto p) {
        scatter_vis_kernel<decltype(p)::value><<<kimg_divup(num_vis, 256), 256, 0, stream>>>(
            b.index, num_vis, b.vis, static_cast<float2 *>(vis)); });
    return kimg_launch_status();
}

extern "C" size_t kimg_grid_binned_workspace_bytes(int64_t max_vis, int num_polarizations,
                                                  int w_planes, int oversample, int kernel_width)
{
    return binned_workspace_bytes(max_vis, num_polarizations, w_planes, oversample, kernel_width,
                                  false);
}

extern "C" size_t kimg_degrid_binned_workspace_bytes(int64_t max_vis, int num_polarizations,
                                                    int w_planes, int oversample, int kernel_width)
{
    return binned_workspace_bytes(max_vis, num_polarizations, w_planes, oversample, kernel_width,
                                  true);
}

extern "C" int kimg_grid_jumps(const int16_t *uv, int64_t num_vis, int kernel_width,
                               uint32_t *count, void *stream)
{
    KIMG_CHECK_ARG(uv && count && num_vis >= 0 && kernel_width >= 1);
    hipStream_t s = (hipStream_t) stream;
    KIMG_HIP(hipMemsetAsync(count, 0, sizeof(uint32_t), s));
    if (num_vis < 2)
        return 0;
    int blocks = kimg_divup(num_vis, 256 * 16);
    if (blocks > 2048)
        blocks = 2048;
    const int slack = kernel_width > 2 * WIN ? 0 : window_slack(kernel_width);
    jump_count_kernel<<<blocks, 256, 0, s>>>(uv, num_vis, slack, count);
    return kimg_launch_status();
}

// (kimg_preload, api.hip)
KIMG_PRELOAD_THIS_UNIT(bin_key_kernel)
