// Shared helpers for the libkimg HIP sources (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "../../include/kimg.h"

#define KIMG_CHECK_ARG(cond) do { if (!(cond)) return KIMG_EINVAL; } while (0)

// Return the negated hipError_t of the last launch on failure.
static inline int kimg_launch_status()
{
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : -(int) e;
}

#define KIMG_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return -(int) e_; } while (0)

static inline int kimg_divup(int64_t a, int64_t b) { return (int) ((a + b - 1) / b); }

// CUs the window kernels (gridder, degridder) may fill with their resident workgroups
// (kimg_set_window_cus; api.hip)
int kimg_window_cus_now();
// (set for the duration of one kimg_grid / kimg_degrid call, on the calling thread)
struct kimg_window_cus_scope {
    explicit kimg_window_cus_scope(int cus);
    ~kimg_window_cus_scope();
    int before;
};

// hipFuncAttributeMaxDynamicSharedMemorySize of kernel `fn` on the current device raised to `bytes`
// (never lowered), once per kernel and device, under one lock (api.hip): channels imaged on several
// host threads reach their first launches together, and two threads setting the attribute of one
// kernel -- or one setting it while the other launches it -- is what their first pass must not do.
int kimg_dynamic_lds(const void *fn, size_t bytes);

// The stream graphs are captured on: one per host thread, the library's own.  A caller's stream is
// never put into capture mode -- streams can be shared between threads without either knowing
// (torch hands out the streams of a pool of 32 per device round robin), and what another thread
// launches on a capturing stream is recorded into the graph instead of run: its kernels never happen,
// and happen later, with its pointers, whenever the graph is launched.  (api.hip)
hipStream_t kimg_capture_stream();

// One kernel of every translation unit (= code object) of the library, for kimg_preload (api.hip):
// returns 0 so that a namespace-scope initialiser can call it.
int kimg_register_kernel(const void *fn);
// ... and a function that launches an empty kernel of the translation unit on the null stream: the
// one thing that is certain to make the runtime load the code object
int kimg_register_touch(void (*launch)());
#define KIMG_PRELOAD_THIS_UNIT(kernel) \
    namespace { __global__ void kimg_touch_kernel() {} \
                void kimg_touch_launch() { kimg_touch_kernel<<<1, 1, 0, nullptr>>>(); } } \
    static const int kimg_preload_registered = \
        kimg_register_kernel(reinterpret_cast<const void *>(&kernel)) + kimg_register_touch(&kimg_touch_launch);

// The multi-component form of the CLEAN loop (clean_multi.hip), reached through kimg_clean_cycles
int kimg_clean_multi_components(int patch_width, int patch_height, int tiles_x, int tiles_y);
size_t kimg_clean_multi_state_bytes(int tiles_x, int tiles_y);
int kimg_clean_multi_run(float *dirty, float *model, int64_t row_stride, int64_t pol_stride,
                         int width, int height, int num_polarizations, const float *psf,
                         int64_t psf_row_stride, int64_t psf_pol_stride, int psf_width,
                         int psf_height, int patch_width, int patch_height, int border, int mode,
                         float loop_gain, float threshold, float *tile_max, int32_t *tile_pos,
                         int tiles_x, int tiles_y, int max_cycles, int components, int repeats,
                         bool relative, double noise_threshold, double left_for_next,
                         void *state, float *log, hipStream_t s, int *cycles_done = nullptr,
                         float *first_peak = nullptr);

// ---- the gridding family (grid.hip, grid_f64.hip, grid_mfma.hip, degrid_mfma.hip, grid_binned.hip) ----
// The float32 window kernels over a stream as given (grid_mfma.hip, degrid_mfma.hip)
int kimg_grid_mfma(void *grid, int64_t grid_row_stride, int64_t grid_pol_stride, int grid_size,
                   int P, const float *weights_grid, int64_t wg_row_stride, int64_t wg_pol_stride,
                   const int16_t *uv, const int16_t *w_plane, const void *vis, int64_t num_vis,
                   const void *convolve_kernel, int w_planes, int oversample, int kernel_width,
                   void *workspace, size_t workspace_bytes, int arith, hipStream_t stream,
                   const void *fold_plan = nullptr, const void *fold_map = nullptr);
bool kimg_grid_mfma_supported(int P, int w_planes, int oversample, int kernel_width);
size_t kimg_grid_mfma_workspace_bytes(int P, int w_planes, int oversample, int kernel_width);
// What kimg_grid_mfma needs ON TOP of the above to run the fold pre-pass on num_vis records, and the
// length from which it does so unasked
size_t kimg_grid_prefold_workspace_bytes(int64_t num_vis, int P);
int64_t kimg_grid_prefold_min_vis();
int kimg_degrid_mfma(const void *grid, int64_t grid_row_stride, int64_t grid_pol_stride,
                     int grid_size, int P, const int16_t *uv, const int16_t *w_plane,
                     const float *weights, void *vis, int64_t num_vis, const void *convolve_kernel,
                     int w_planes, int oversample, int kernel_width, void *workspace,
                     size_t workspace_bytes, int arith, hipStream_t stream);
bool kimg_degrid_mfma_supported(int P, int w_planes, int oversample, int kernel_width);
size_t kimg_degrid_mfma_workspace_bytes(int P, int w_planes, int oversample, int kernel_width);
// The fold pre-pass (grid_fold.hip): runs of consecutive records with equal (u, v, sub_u, sub_v,
// w_plane) compacted into one record each, with the sum of their samples.  Its header, in device
// memory at the start of its workspace, is what the window gridder's kernel reads: whether to grid
// the compacted stream, how long it is and where it lies.
struct kimg_fold_header {
    uint32_t use_folded;            // 0: grid the caller's stream (nothing else below is valid)
    uint32_t spans;                 // workgroups' spans the stream was cut into
    int64_t count;                  // H, heads of runs (whether or not they were written)
    const int16_t *uv, *w_plane;    // the compacted stream: `count` records
    const float2 *vis;              //   [count][P]
    int64_t capacity;
    uint32_t reserved[4];
    // calls with a fold plan only: spans that have finished (bits 0-15) and spans whose own count of
    // heads was not the plan's (bits 16-31); a 16-byte block that the call zeroes ahead of its launch
    uint32_t ticket[4];
};
// A fold plan (kimg_fold_plan, include/kimg.h): what the count launch of the pre-pass finds out about
// one (uv, w_plane, num_vis, P) stream, kept by the caller in device memory.  Untrusted where it is
// used: see fold_compact_kernel.
constexpr int KIMG_FOLD_MAX_SPANS = 1024;
constexpr uint32_t KIMG_FOLD_PLAN_MAGIC = 0x31504c46u;     // "FLP1"
struct kimg_fold_plan_data {
    uint32_t magic, spans;          // the layout the counts belong to: fold_plan_of(num_vis, P)
    int64_t num_vis, tiles_per_span;
    int64_t count;                  // H, the sum of the counts
    uint32_t reserved[8];
    uint32_t counts[KIMG_FOLD_MAX_SPANS];   // heads of runs per span
};
// A fold map (kimg_fold_map, include/kimg.h): what the pre-pass derives from uv and w_plane alone,
// kept by the caller in device memory -- this block, then one byte of head bits per 8 records (a
// thread's fold_heads; padded to 16 bytes), then the compacted uv (int2 [H], H rounded up to 8) and
// w_plane (int16 [H]).  Trusted for results once `valid` is set, never for addresses: see
// fold_compact_kernel.
constexpr uint32_t KIMG_FOLD_MAP_MAGIC = 0x314d4c46u;      // "FLM1"
struct kimg_fold_map_data {
    uint32_t magic, spans;          // as in the plan it was made from
    int64_t num_vis, tiles_per_span;
    int64_t count;                  // H
    int64_t heads;                  // records the buffer has room for
    uint32_t valid;                 // 1: every span found the plan's count when the map was made
    uint32_t reserved;
    uint32_t ticket[4];             // (of the launch that fills the map, as kimg_fold_header's)
    uint32_t counts[KIMG_FOLD_MAX_SPANS];
};
size_t kimg_fold_workspace_bytes(int P, int64_t capacity);
// (16-byte aligned uv, w_plane, vis and workspace; workspace of at least the size above; `plan`: null
// or a fold plan in device memory, which replaces the count launch; `map`: null or a fold map, which
// replaces the key loads and the compacted coordinates as well, and comes before a plan)
int kimg_fold_launch(const int16_t *uv, const int16_t *w_plane, const float2 *vis, int64_t num_vis,
                     int P, int64_t capacity, void *workspace, hipStream_t stream,
                     const kimg_fold_plan_data *plan = nullptr,
                     const kimg_fold_map_data *map = nullptr);
// *out = the bit pattern of the largest |component| among the n floats of a kernel table (ktable.hip):
// the fp16 hi/lo forms of the window kernels choose their table scale from it when the table is in
// HBM.  (Hidden: a helper between two units of the library, no part of its dynamic symbol table.)
__attribute__((visibility("hidden")))
int kimg_table_max(const float *kern, int64_t n, unsigned *out, hipStream_t stream);
// ... and the float64 ones (grid_f64.hip)
int kimg_grid_window_f64(double *grid, int64_t grid_row_stride, int64_t grid_pol_stride,
                         int grid_size, int P, const float *weights_grid, int64_t wg_row_stride,
                         int64_t wg_pol_stride, const int16_t *uv, const int16_t *w_plane,
                         const float2 *vis, int64_t num_vis, const float2 *kern, int w_planes,
                         int oversample, int K, hipStream_t s);
int kimg_degrid_window_f64(const double2 *grid, int64_t grid_row_stride, int64_t grid_pol_stride,
                           int grid_size, int P, const int16_t *uv, const int16_t *w_plane,
                           const float *weights, float2 *vis, int64_t num_vis, const float2 *kern,
                           int w_planes, int oversample, int K, hipStream_t s);

// KIMG_VARIANT_BINNED (grid_binned.hip): the stream in tile order, inside the caller's workspace
// (kimg_grid_binned_workspace_bytes / kimg_degrid_binned_workspace_bytes), for a window kernel to run on
struct kimg_binned_stream {
    const int16_t *uv, *w_plane;
    float2 *vis;
    float *weights;                 // degridders only
    const unsigned *index;          // the caller's record of sorted place i
    void *table;                    // the float32 window kernel's own scratch
    size_t table_bytes;
};
// `weights` null: a gridder's stream (no weights gathered, the gridder's workspace layout)
int kimg_bin_stream(const int16_t *uv, const int16_t *w_plane, const float *weights, const void *vis,
                    int64_t num_vis, int grid_size, int P, int w_planes, int oversample,
                    int kernel_width, void *workspace, size_t workspace_bytes, hipStream_t stream,
                    kimg_binned_stream &out);
// a degridder's results back in the caller's order
int kimg_unbin_vis(const kimg_binned_stream &b, void *vis, int64_t num_vis, int P, hipStream_t stream);

// f(std::integral_constant<int, P>{}) for the runtime P in 1..4 (callers have checked the range)
template <class F> inline void kimg_for_pols(int P, F &&f)
{
    switch (P) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    }
}

// f(std::integral_constant<int, MODE>{}) for KIMG_CLEAN_I / KIMG_CLEAN_SUMSQ; false (and no call) for
// any other mode
template <class F> inline bool kimg_for_clean_mode(int mode, F &&f)
{
    switch (mode) {
    case KIMG_CLEAN_I: f(std::integral_constant<int, KIMG_CLEAN_I>{}); return true;
    case KIMG_CLEAN_SUMSQ: f(std::integral_constant<int, KIMG_CLEAN_SUMSQ>{}); return true;
    }
    return false;
}

constexpr int WAVE = 64;    // gfx950 wavefront

// Wave-wide sum by DPP-backed shuffles; result valid in every lane.
__device__ inline float wave_sum(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_xor(v, off, WAVE);
    return v;
}

__device__ inline double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_xor(v, off, WAVE);
    return v;
}

// One record of the uv stream: (u, v, sub_u, sub_v) as four int16
struct vis_coord {
    int u, v, sub_u, sub_v;
};

__device__ inline vis_coord load_uv(const int16_t *__restrict__ uv, int64_t i)
{
    const int2 packed = reinterpret_cast<const int2 *>(uv)[i];
    vis_coord c;
    c.u = (short) (packed.x & 0xffff);
    c.v = (short) (packed.x >> 16);
    c.sub_u = (short) (packed.y & 0xffff);
    c.sub_v = (short) (packed.y >> 16);
    return c;
}

// A record whose cell, sub-cell or plane lies outside the grid / table contributes nothing (the
// window kernel's coords_ok, grid_mfma.hip).
__device__ inline bool coords_ok(const vis_coord &c, int wp, int Gg, int w_planes, int oversample)
{
    const int half = Gg / 2;
    return (unsigned) (c.u + half) < (unsigned) Gg && (unsigned) (c.v + half) < (unsigned) Gg
           && (unsigned) c.sub_u < (unsigned) oversample && (unsigned) c.sub_v < (unsigned) oversample
           && (unsigned) wp < (unsigned) w_planes;
}
