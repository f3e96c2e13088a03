/* libkimg -- C ABI of the MI355X (gfx950) imaging hot path.
 *
 * Drop-in boundary for the per-channel imaging loop of ska-sa/katsdpimager:
 * each entry point replaces one device-kernel launch site of the reference's
 * operator classes (file:line relative to the reference checkout).  The
 * reference reaches its kernels through katsdpsigproc's
 * `command_queue.enqueue_kernel(...)`; a maintainer binds these functions with
 * ctypes/cffi instead.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller unless the name
 *    ends in `_host`; nothing is allocated or freed here except FFT plans;
 *  - arrays come with explicit element strides (row, polarization) exactly
 *    like the reference kernels' arguments;
 *  - a row stride below the row's width is KIMG_EINVAL, before anything is enqueued;
 *  - a pointer needs only the alignment of its element type unless its argument says otherwise;
 *  - `stream` is a hipStream_t (NULL = default stream); all calls are
 *    asynchronous on it and may be captured into a hipGraph unless noted;
 *  - return value: 0 on success, a negated hipError_t on a HIP failure, or a
 *    KIMG_E* code below for argument errors.  Kernels themselves never report
 *    errors (same as the reference).
 *  - complex numbers are interleaved float (re, im) = numpy complex64; the `_f64` entry points
 *    take complex128 / float64 grids, layers and images (see "float64 path" below).
 */
#ifndef KIMG_H
#define KIMG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KIMG_VERSION 5

#define KIMG_EINVAL (-10001)      /* bad argument (null pointer, negative size ...) */
#define KIMG_EUNSUPPORTED (-10002) /* parameter combination not supported by this build */
#define KIMG_EWORKSPACE (-10003)   /* workspace too small */
#define KIMG_ETIMEOUT (-10004)     /* the host-paced loop of KIMG_CLEAN_FORM_MULTI saw no progress of the
                                    * device in time (the return value of the call) */

/* Arithmetic of the gridder / degridder matrix instructions (argument `arith`):
 *   KIMG_ARITH_FP32        every product and sum in float32, bit-identical to the fmaf chain of the
 *                          reference's kernels (grid.py:1049-1052).  Default.  The gridder runs it
 *                          on v_mfma_f32_16x16x4_f32, two visibilities per instruction; the
 *                          degridder on v_mfma_f32_32x32x2_f32.
 *   KIMG_ARITH_SPLIT_FP16  operands carried as fp16 (hi, lo) pairs (22 significant bits, lo*lo
 *                          dropped), two visibilities per v_mfma_f32_32x32x16_f16, float32
 *                          accumulation.  Faster, narrower than the reference's arithmetic: opt-in.
 *   KIMG_ARITH_FP32_32X32  the same sums as KIMG_ARITH_FP32, the gridder on v_mfma_f32_32x32x2_f32
 *                          (one visibility per instruction; the earlier default form, kept for
 *                          comparison).  Gridder only: the degridder rejects it (KIMG_EINVAL).
 * The generic (non-MFMA) kernels always compute in float32 and ignore it.
 *
 * One exception to "bit-identical", in every form of the window gridder (kimg_grid, MFMA and binned
 * variants): consecutive records of one call with equal (u, v, sub_u, sub_v, w_plane) add the same
 * rank-1 matrix to the grid, and the gridder may sum their weighted samples (vis * weights_grid) in
 * float32, in unspecified order, and apply ONE update with the sum -- what the reference's
 * preprocessor does to such runs before its gridder sees them.  How long a folded run is is not
 * part of the contract (runs are cut wherever the kernel's batches end).  A stream without adjacent
 * duplicates is gridded exactly as before.
 * Long calls (and calls with KIMG_ARITH_PREFOLD) whose workspace has the room fold such runs in a
 * pass of its own ahead of the window kernel (kimg_fold_runs below), which sums the RAW samples of a
 * run in float32; the window kernel then weights the sum: weights_grid * sum(vis) in place of
 * sum(vis * weights_grid) -- all records of a run read the same weight.  Both are allowed.
 *   KIMG_ARITH_NO_FOLD     a bit OR-ed into any of the above (kimg_grid only): every record gets its
 *                          own update, as before the fold existed.  For comparison and tests.
 *   KIMG_ARITH_PREFOLD     a bit OR-ed into any of the forms (kimg_grid only): the MFMA variant takes
 *                          the fold pre-pass whatever the number of records, when the workspace has
 *                          room for it (see `workspace` of kimg_grid); without the bit only calls
 *                          long enough for it to pay do.  For comparison and tests.  Together with
 *                          KIMG_ARITH_NO_FOLD it is KIMG_EINVAL.  (0x400, not the next free bit:
 *                          0x200 alone stays an invalid `arith`, as callers have been told.)
 *   KIMG_ARITH_NO_PREFOLD  a bit OR-ed into any of the forms (kimg_grid only): the call does not take
 *                          the fold pre-pass whatever the number of records -- for a caller that
 *                          has measured its stream (kimg_fold_plan) and knows that it does not fold.
 *                          The window kernel still folds the runs it meets.  A fold plan given with
 *                          it is ignored; together with KIMG_ARITH_PREFOLD it is KIMG_EINVAL. */
#define KIMG_ARITH_FP32 0
#define KIMG_ARITH_SPLIT_FP16 1
#define KIMG_ARITH_FP32_32X32 2
#define KIMG_ARITH_NO_FOLD 0x100
#define KIMG_ARITH_PREFOLD 0x400
#define KIMG_ARITH_NO_PREFOLD 0x800

/* Kernel choice of kimg_grid / kimg_degrid (argument `variant`) */
#define KIMG_VARIANT_AUTO 0     /* MFMA window kernel when the parameters allow it */
#define KIMG_VARIANT_GENERIC 1  /* one wave per visibility, any kernel width */
#define KIMG_VARIANT_MFMA 2     /* MFMA window kernel or KIMG_EUNSUPPORTED */
#define KIMG_VARIANT_BINNED 3   /* sort the visibilities by grid tile on the device
                                 * (bins of window-slack cells, stable radix sort, gather), then the
                                 * MFMA window kernel over the sorted copies -- for streams without
                                 * locality (time order, shuffled); needs the scratch of
                                 * kimg_grid_binned_workspace_bytes / kimg_degrid_binned_workspace_bytes
                                 * (the degridder also sorts the weights and scatters its results
                                 * back into the caller's order); KIMG_EUNSUPPORTED where MFMA is */

/* Form of the device-resident CLEAN loop (argument `form` of kimg_clean_cycles) */
#define KIMG_CLEAN_FORM_AUTO 0      /* one launch per cycle when the patch's lattice blocks fit the CUs */
#define KIMG_CLEAN_FORM_TWO_LAUNCH 1
#define KIMG_CLEAN_FORM_ONE_LAUNCH 2    /* falls back to two launches when the patch is too large */
#define KIMG_CLEAN_FORM_PERSISTENT 3    /* retired: measured slower, runs as ONE_LAUNCH */
#define KIMG_CLEAN_FORM_ONE_WORKGROUP 4 /* retired: measured slower, runs as ONE_LAUNCH */

#define KIMG_CLEAN_FORM_MULTI 5     /* SEVERAL components per launch: a launch verifies the components
                                     * the last one evaluated speculatively, commits the verified
                                     * prefix and evaluates the next up to 8 (csrc/clean_multi.hip);
                                     * results bit-identical to the other forms.  At most 256 lattice
                                     * blocks per patch (8 components per launch up to 32 blocks, 4
                                     * up to 64, 2 up to 128) and 2047 tiles per axis; falls back to
                                     * AUTO's other choices otherwise.  A planned component may be
                                     * stepped several times in a launch (its peak's value follows a
                                     * scalar recursion every workgroup evaluates; up to 8 steps, 4
                                     * with several polarizations).  `form | n << 8` caps the
                                     * components per launch at n (1..8), `| r << 16` the steps per
                                     * component at r (1..8; the loop goes over to repeated steps
                                     * only while it sees few components per launch: `| 1 << 20`
                                     * makes it take them from the first launch on).  AUTO takes this form when
                                     * at least 2 components fit and at least 4 cycles are asked for.
                                     * HOST-PACED: the number of launches depends on the data, so the
                                     * call watches a progress word the device writes and returns
                                     * once the loop has ended -- it blocks the calling thread for
                                     * about as long as the loop runs, and cannot be captured. */

#define KIMG_CLEAN_I 0      /* clean.py:29 */
#define KIMG_CLEAN_SUMSQ 1  /* clean.py:31 */

int kimg_version(void);

/* Load every code object of the library on the current device now, in the calling thread.  The runtime
 * otherwise loads a code object at the first launch of one of its kernels, and first launches that
 * several host threads make at the same moment (channels imaged concurrently) are not safe against
 * that load: call this once per device before any thread uses the library.  Idempotent. */
int kimg_preload(void);
/* Static string describing a return code of this library. */
const char *kimg_error_string(int code);
/* How many of the device's CUs the window kernels (kimg_grid / kimg_degrid, MFMA variants) fill with
 * their resident workgroups: 256 (all; the default, also set by 0) down to 1.  Process-wide, takes
 * effect with the next launch.  A process that keeps several channels in flight on one GPU
 * (frontend.process_channel_stream) sets 192: the window kernels' workgroups stay for a whole launch
 * (0.7 ms on a stored W-slice) and leave no room for another channel's CLEAN workgroups (1024
 * threads, 64 KB of LDS), whose latency-bound chain then stands still; with 64 CUs left free a
 * 12-channel stream with four in flight takes 6.1 instead of 7.2 ms per channel, one channel alone
 * 16.1 instead of 15.6.  No counterpart in the reference (its kernels are not resident). */
int kimg_set_window_cus(int cus);
int kimg_get_window_cus(void);
/* The same PER CALL, which is what callers should use (the process-wide setting above is kept as
 * the default for calls that bring none, and is deprecated: two imagers of one process with
 * different needs would race on it): `variant | KIMG_WINDOW_CUS(n)` in the `variant` argument of
 * kimg_grid / kimg_degrid, n = 1 .. 256; 0 = the default. */
#define KIMG_WINDOW_CUS(n) ((n) << 8)

/* ---- convolution kernel table: grid.py:235-334 antialias_w_kernel, as called for every W plane
 * by ConvolutionKernel.__init__ (grid.py:358-389), evaluated on the device in float64.
 *   table  complex64 [w_planes][oversample][kernel_width] (device, written)
 *   ws     float64 [w_planes] (device): the w of each plane in wavelengths, grid.py:382-383
 *   beta   Kaiser-Bessel shape parameter, grid.py:374-378
 * table[w][s][t] = sample t*oversample + (oversample-1-s) of the central oversample*kernel_width
 * samples of step * FFT(ifftshift(aa(l) exp(2 pi i (-w (-l^2/2 - 5 l^4/24) + half_subcell l)))),
 * l on an image_oversample-times finer grid of step 1/(kernel_width cell_wavelengths
 * image_oversample).  oversample*kernel_width must be even (KIMG_EINVAL, grid.py:268);
 * KIMG_EUNSUPPORTED when oversample*kernel_width*image_oversample > 5120 (the plane's samples and
 * the roots of unity are kept in LDS). */
int kimg_kernel_table(void *table, const double *ws, int w_planes, int kernel_width,
                      int oversample, int image_oversample, double cell_wavelengths,
                      double antialias_width, double beta, void *stream);

/* ---- gridding: grid.py:786-867 Gridder.static_run/_run + imager_kernels/grid.mako:63-197
 * grid[p][v0+j][u0+k] += vis[r][p] * weights_grid[p][v+Gg/2][u+Gg/2]
 *                        * conj(kern[w][sub_v][j] * kern[w][sub_u][k]),
 * u0 = u - ((K-1)/2 - Gg/2)  (grid.py:1038-1041).
 *   grid            complex64 [P][grid_size][grid_size] (strides in complex elements)
 *   weights_grid    float32   [P][grid_size][grid_size] (strides in elements)
 *   uv              int16 [N][4] = (u, v, sub_u, sub_v)       grid.py:661-664
 *   w_plane         int16 [N]
 *   vis             complex64 [N][P]
 *   convolve_kernel complex64 [w_planes][oversample][kernel_width], unpadded
 *   workspace       device scratch, at least kimg_grid_workspace_bytes(max N, P, w_planes,
 *                   oversample, kernel_width) bytes: 256 bytes (the chunk counter from which the
 *                   waves of a long launch draw their work; without it -- NULL is accepted when the
 *                   table fits LDS -- they take their chunks in a fixed order, a few per cent slower)
 *                   plus, when the kernel table is too large for LDS -- more than 512 rows
 *                   w_planes*oversample for widths <= 32, 256 for 33..64 -- a zero-padded copy of it,
 *                   built there on every call.  One call at a time per workspace.
 *                   For max N of 8 Mi records or more the size includes room for the fold pre-pass:
 *                   kimg_fold_runs_workspace_bytes(P, max N / 2) more.  A call on N records takes
 *                   the pre-pass when workspace_bytes is at least kimg_grid_workspace_bytes(0, ...)
 *                   + kimg_fold_runs_workspace_bytes(P, N / 2), uv, w_plane, vis and workspace are
 *                   16-byte aligned, and N >= 8 Mi or KIMG_ARITH_PREFOLD is set or a fold plan is
 *                   given (kimg_grid_planned); with less -- the sizes of before the pre-pass
 *                   existed, or NULL -- it silently goes without.
 *   variant         KIMG_VARIANT_*: automatic = MFMA window kernel when supported (kernel_width
 *                   <= 64), else the generic scatter kernel
 *   arith           KIMG_ARITH_* (above); anything else is KIMG_EINVAL
 *   Out-of-range coordinates (footprint outside the grid, sub_uv >= oversample, w_plane >=
 *   w_planes) contribute nothing instead of faulting.
 */
size_t kimg_grid_workspace_bytes(int64_t max_vis, int num_polarizations, int w_planes,
                                 int oversample, int kernel_width);
/* Scratch of kimg_grid with KIMG_VARIANT_BINNED (includes the above): sort keys and indices, the
 * sorted copies of uv / w_plane / vis (18 + 8 P bytes per visibility) and the sort's own scratch. */
size_t kimg_grid_binned_workspace_bytes(int64_t max_vis, int num_polarizations, int w_planes,
                                        int oversample, int kernel_width);
/* How well a visibility stream suits the window kernel: *count (device uint32, zeroed by the call)
 * receives the number of records whose (u, v) cell differs from their predecessor's by more than
 * the window slack (32 - kernel_width; 32 - (kernel_width + 1) / 2 for widths 33..64) along
 * either axis: each of them costs a whole-window flush in the direct window kernel.  A caller may
 * choose KIMG_VARIANT_BINNED when count / num_vis is more than a few percent. */
int kimg_grid_jumps(const int16_t *uv, int64_t num_vis, int kernel_width, uint32_t *count,
                    void *stream);
/* The fold pre-pass of kimg_grid on its own: runs of consecutive records with equal (u, v, sub_u,
 * sub_v, w_plane) become one record each, with the float32 sum of the run's samples per polarization,
 * in stream order (deterministic).  Runs are also cut at the boundaries of up to 1024 contiguous
 * spans the stream is divided into, and nowhere else.  Two launches, asynchronous, capturable.
 *   uv, w_plane, vis  as for kimg_grid, N >= 1 records, each pointer 16-byte aligned
 *   capacity          records the output may hold
 *   workspace         device memory, 16-byte aligned, kimg_fold_runs_workspace_bytes(P, capacity)
 *                     bytes.  At its start a header: uint32 use_folded, uint32 spans, int64 H (the
 *                     number of heads of runs), then three device pointers into the workspace --
 *                     the compacted uv int16 [H][4], w_plane int16 [H], vis complex64 [H][P] -- and
 *                     int64 capacity.  (Further words of the first 256 bytes belong to the library.)
 * If 2 H > N (folding would not halve the stream) or H > capacity, use_folded is 0 and no record is
 * written; else use_folded is 1 and the H records are there.
 * KIMG_EINVAL for null or misaligned pointers and N < 1, KIMG_EWORKSPACE for a short workspace. */
size_t kimg_fold_runs_workspace_bytes(int num_polarizations, int64_t capacity);
int kimg_fold_runs(const int16_t *uv, const int16_t *w_plane, const void *vis, int64_t num_vis,
                   int num_polarizations, int64_t capacity, void *workspace, size_t workspace_bytes,
                   void *stream);
int kimg_grid(void *grid, int64_t grid_row_stride, int64_t grid_pol_stride, int grid_size,
              int num_polarizations,
              const float *weights_grid, int64_t wg_row_stride, int64_t wg_pol_stride,
              const int16_t *uv, const int16_t *w_plane, const void *vis, int64_t num_vis,
              const void *convolve_kernel, int w_planes, int oversample, int kernel_width,
              void *workspace, size_t workspace_bytes, int variant, int arith, void *stream);
/* Fold plans: the count launch of the pre-pass run ONCE for a stream that is gridded several times.
 * The heads of runs depend on uv and w_plane alone, and a slice is gridded with the same coordinates
 * for the PSF, for the dirty image and in every major cycle; only vis changes.
 *   kimg_fold_plan_bytes()  size of a plan: a small fixed number of bytes of device memory, 16-byte
 *                           aligned.  Its first words: uint32 magic, uint32 spans, int64 num_vis,
 *                           int64 tiles per span, int64 H (the heads of runs kimg_fold_runs would
 *                           count), so a caller can read H back (32 bytes) and decide.
 *   kimg_fold_plan          fills `plan` for (uv, w_plane, N >= 1, P): two launches, asynchronous,
 *                           capturable, no allocation.  The plan depends on P because the spans do.
 *   kimg_fold_runs_planned  kimg_fold_runs with the counts taken from `fold_plan`: one launch (and
 *                           a 16-byte memset).  NULL: kimg_fold_runs.
 *   kimg_grid_planned       kimg_grid with `fold_plan` for the MFMA variant's pre-pass, which is
 *                           then taken at ANY N (room in the workspace and alignment as always):
 *                           the plan is the caller's statement that the stream folds, so give one
 *                           only when 2 H <= N, and KIMG_ARITH_NO_PREFOLD otherwise.  The generic
 *                           and binned variants, KIMG_ARITH_NO_FOLD and KIMG_ARITH_NO_PREFOLD
 *                           ignore it.  NULL: kimg_grid.
 * A STALE PLAN NEVER CHANGES THE RESULT.  A plan is untrusted device data, which the host cannot
 * read: the pre-pass counts every span's heads again while it compacts, and only if the plan was made
 * for this N and span layout and every span's count is the plan's does use_folded become 1 -- then
 * the output is bit for bit what the unplanned call writes.  Otherwise (coordinates rewritten in
 * place, the plan of another stream, another P-layout, arbitrary bytes) use_folded is 0 and kimg_grid
 * grids the caller's stream; records may then have been written, but whatever the plan holds nothing
 * is written outside the workspace.  The decision is taken on the device, without a read-back.  All
 * the host checks is the pointer: KIMG_EINVAL for a plan that is not 16-byte aligned. */
size_t kimg_fold_plan_bytes(void);
int kimg_fold_plan(const int16_t *uv, const int16_t *w_plane, int64_t num_vis, int num_polarizations,
                   void *plan, void *stream);
int kimg_fold_runs_planned(const int16_t *uv, const int16_t *w_plane, const void *vis,
                           int64_t num_vis, int num_polarizations, int64_t capacity, void *workspace,
                           size_t workspace_bytes, void *stream, const void *fold_plan);
/* (kimg_grid's arguments in kimg_grid's order -- the four after `grid` and `weights_grid` are its
 * row and polarization strides, refused alike -- then the plan) */
int kimg_grid_planned(void *grid, int64_t grid_row, int64_t grid_pol, int grid_size,
                      int num_polarizations,
                      const float *weights_grid, int64_t wg_row, int64_t wg_pol,
                      const int16_t *uv, const int16_t *w_plane, const void *vis, int64_t num_vis,
                      const void *convolve_kernel, int w_planes, int oversample, int kernel_width,
                      void *workspace, size_t workspace_bytes, int variant, int arith, void *stream,
                      const void *fold_plan);
/* Fold maps: everything the pre-pass derives from uv and w_plane, kept across calls.  Besides the
 * counts that is which records head a run and the compacted coordinates; a call that is given a
 * map reads the samples and one bit per record and writes the sums -- no key is read or compared,
 * no coordinate written.  A map costs N / 8 + 10 H bytes of device memory (plus 4160).
 *   kimg_fold_map_bytes     size of a map of N records with room for `heads` runs (0 for arguments
 *                           out of range).  Take `heads` from the plan's H.
 *   kimg_fold_map           fills `map` (device memory, 16-byte aligned, map_bytes long) from the
 *                           stream and its `fold_plan`: one launch (and a 16-byte memset),
 *                           asynchronous, capturable, no read-back.  The layout is private.  The
 *                           launch counts every span's heads again; the map is marked valid only
 *                           if the plan was made for this N and layout, every span found the
 *                           plan's count and H fits map_bytes -- a stale plan makes a map that
 *                           every call refuses.  KIMG_EWORKSPACE: map_bytes below
 *                           kimg_fold_map_bytes(N, P, 0).
 *   kimg_fold_runs_mapped   kimg_fold_runs with `fold_map`: one launch.  The header's uv and
 *                           w_plane then point INTO THE MAP, vis into the workspace.  The sums are
 *                           bit for bit those of kimg_fold_runs_planned, for any samples: the same
 *                           additions in the same order.  NULL: kimg_fold_runs.
 *   kimg_grid_mapped        kimg_grid with `fold_map` for the MFMA variant's pre-pass, at any N,
 *                           under the conditions of kimg_grid_planned.  NULL: kimg_grid.
 * UNLIKE A PLAN, A MAP IS BELIEVED.  It belongs to the exact bytes of uv[0..N) and w_plane[0..N) it
 * was made from, and the calls do not look at them again:
 *   - a map of another N or span layout (another P may be one), one that was never valid, one
 *     whose H exceeds the capacity (N / 2 for kimg_grid_mapped) and arbitrary bytes are refused on
 *     the device: use_folded is 0 and kimg_grid grids the caller's stream.  That costs time only.
 *   - a valid map whose coordinates have since been rewritten in place gives a WRONG grid: make a
 *     new plan and map after changing uv or w_plane.
 *   - in no case, junk included, does a map cause a write outside the workspace or the grid: every
 *     sum's index is checked against the capacity, and the window kernel range-checks the
 *     compacted coordinates like any caller's.
 * KIMG_EINVAL for a map that is not 16-byte aligned. */
size_t kimg_fold_map_bytes(int64_t num_vis, int num_polarizations, int64_t heads);
int kimg_fold_map(const int16_t *uv, const int16_t *w_plane, int64_t num_vis, int num_polarizations,
                  const void *fold_plan, void *map, size_t map_bytes, void *stream);
int kimg_fold_runs_mapped(const int16_t *uv, const int16_t *w_plane, const void *vis,
                          int64_t num_vis, int num_polarizations, int64_t capacity, void *workspace,
                          size_t workspace_bytes, void *stream, const void *fold_map);
int kimg_grid_mapped(void *grid, int64_t grid_row, int64_t grid_pol, int grid_size,
                     int num_polarizations,
                     const float *weights_grid, int64_t wg_row, int64_t wg_pol,
                     const int16_t *uv, const int16_t *w_plane, const void *vis, int64_t num_vis,
                     const void *convolve_kernel, int w_planes, int oversample, int kernel_width,
                     void *workspace, size_t workspace_bytes, int variant, int arith, void *stream,
                     const void *fold_map);

/* ---- degridding: grid.py:985-1029 Degridder.static_run/_run + degrid.mako:77-199
 * vis[r][p] -= weights[r][p] * sum_{j,k} kern[w][sub_v][j]*kern[w][sub_u][k]*grid[p][v0+j][u0+k]
 *   weights  float32 [N][P] statistical weights
 *   variant, arith as for kimg_grid
 */
int kimg_degrid(const void *grid, int64_t grid_row_stride, int64_t grid_pol_stride, int grid_size,
                int num_polarizations,
                const int16_t *uv, const int16_t *w_plane, const float *weights, void *vis,
                int64_t num_vis,
                const void *convolve_kernel, int w_planes, int oversample, int kernel_width,
                void *workspace, size_t workspace_bytes, int variant, int arith, void *stream);
/* Device scratch kimg_degrid needs, as for kimg_grid: 256 bytes (the chunk counter of long launches;
 * optional when the table fits LDS) plus, when the kernel table is too large for LDS, a padded copy
 * of it, built there on every call.  One call at a time per workspace. */
size_t kimg_degrid_workspace_bytes(int num_polarizations, int w_planes, int oversample,
                                   int kernel_width);
/* Scratch of kimg_degrid with KIMG_VARIANT_BINNED (includes the above). */
size_t kimg_degrid_binned_workspace_bytes(int64_t max_vis, int num_polarizations, int w_planes,
                                          int oversample, int kernel_width);

/* ---- float64 path (the reference's --precision double, frontend.py:300): complex128 grid,
 * complex64 visibilities and kernel table, float32 weights_grid and statistical weights.  Arguments
 * as kimg_grid / kimg_degrid without `arith`; `variant` may carry KIMG_WINDOW_CUS(n) (ignored).
 *   grid  complex128 [P][grid_size][grid_size] (strides in complex elements)
 * Arithmetic contract:
 *   gridder    s_p = float32(vis_p * wgt_p), as in the float32 forms; then in double
 *              a_j = s_p * conj(kv_j) (taps promoted exactly) and
 *              grid[p][v0+j][u0+k] += a_j * conj(ku_k).
 *              (The reference's GPU double path rounds kv_j * ku_k to float32 first,
 *              grid.mako:21-35; this separable form differs from it by at most 2^-24 relative
 *              per tap and is the more accurate.)
 *   degridder  in double, pred = sum_k ku_k sum_j kv_j g[j][k] (a separable contraction, either
 *              order), residual = complex64(vis - weight * pred) with one final rounding
 *              (DegridderHost._degrid on complex128 values, grid.py:1139-1154).
 *   The order of summation is free: with integer operands whose partial sums stay below 2^53
 *   both results are exact.  Out-of-range coordinates contribute nothing, as in kimg_grid (the
 *   whole record for a cell, sub-cell or plane outside the grid or table; single taps for a
 *   footprint that crosses the grid's edge).
 * Kernels (csrc/grid_f64.hip): widths up to 32 run a moving 32 x 32 complex128 window held in
 * registers (v_fma_f64; flushes with global_atomic_add_f64 only where the window's mapping changes):
 * KIMG_VARIANT_MFMA, and KIMG_VARIANT_BINNED over the tile-sorted copies of the float32 binned
 * variant (same scratch: kimg_grid_binned_workspace_bytes / kimg_degrid_binned_workspace_bytes).
 * Widths 33 and
 * up run the generic one-wave-per-visibility kernels (no 2 x 2 tap-block split): MFMA and BINNED
 * are KIMG_EUNSUPPORTED there.  AUTO = the window kernel up to 32, generic above; GENERIC = the
 * generic kernels.  Only BINNED needs a workspace (NULL, 0 accepted otherwise). */
int kimg_grid_f64(void *grid, int64_t grid_row_stride, int64_t grid_pol_stride, int grid_size,
                  int num_polarizations,
                  const float *weights_grid, int64_t wg_row_stride, int64_t wg_pol_stride,
                  const int16_t *uv, const int16_t *w_plane, const void *vis, int64_t num_vis,
                  const void *convolve_kernel, int w_planes, int oversample, int kernel_width,
                  void *workspace, size_t workspace_bytes, int variant, void *stream);
int kimg_degrid_f64(const void *grid, int64_t grid_row_stride, int64_t grid_pol_stride,
                    int grid_size, int num_polarizations,
                    const int16_t *uv, const int16_t *w_plane, const float *weights, void *vis,
                    int64_t num_vis,
                    const void *convolve_kernel, int w_planes, int oversample, int kernel_width,
                    void *workspace, size_t workspace_bytes, int variant, void *stream);

/* ---- direct prediction: predict.py:386-416 Predict._run + predict.mako:10-87
 * vis[r][p] -= weights[r][p] * sum_s flux[s][p] * exp(-2 pi i (l u + m v + (n-1) w)),
 * u = (uv.x*oversample + uv.z + 0.5)*uv_scale, w = w_plane*w_scale + w_bias.
 *   lmn float32 [S][3] (l, m, n-1);  flux float32 [S][P]
 * Arithmetic (float32 throughout, fl() = one round to nearest, no contraction unless named):
 *   u_f = fl(fl(uv.x*oversample + uv.z + 0.5) * uv_scale)   (the integer converts exactly below
 *         2^24 and the + 0.5 is exact below 2^23: one rounding);  v_f likewise from uv.y, uv.w
 *   w_f = fl(fl(w_plane*w_scale) + w_bias)
 *   phi = fl(fl(fl(l*u_f) + fl(m*v_f)) + fl((n-1)*w_f))               in turns
 *   t = v_fract_f32(phi) = phi - floor(phi)   (exact but for a tiny negative phi, where it lies
 *         within 2^-24 of 1);  c = v_cos_f32(t), s = v_sin_f32(t)
 *         (argument in turns: c ~ cos(2 pi t), s ~ sin(2 pi t))
 *   acc[p] = fmaf(c, flux[j][p], acc[p]) (re), fmaf(-s, flux[j][p], acc[p]) (im), one rounding
 *         per source, for j = 0 .. S-1 in order from acc = 0 (the LDS chunks of 256 are padded
 *         with zero-flux sources, which add exact zeros)
 *   vis[r][p] = fl(vis[r][p] - fl(acc[p]*weights[r][p]))      re and im separately
 * Nothing at or beyond num_vis is read from weights or written to vis.  num_vis == 0 or
 * num_sources == 0 returns 0 with no launch (lmn, flux may then be NULL).  P outside 1-4:
 * KIMG_EUNSUPPORTED.  There is no float64 form.
 */
int kimg_predict(void *vis, const int16_t *uv, const int16_t *w_plane, const float *weights,
                 const float *lmn, const float *flux, int64_t num_vis, int num_sources,
                 int num_polarizations, int oversample, float uv_scale, float w_scale,
                 float w_bias, void *stream);

/* ---- imaging weights: weight.py:155-176 / 261-284 / 357-376 + grid_weights.mako,
 * density_weights.mako, mean_weight.mako; fill = katsdpsigproc fill.FillTemplate (weight.py:403).
 *   kimg_grid_weights:    grid[p][v+H/2][u+W/2] += weights[r][p]   (uv = first 2 of 4 int16)
 *   kimg_mean_weight:     sums[0] = sum w, sums[1] = sum w^2 over polarization 0
 *   kimg_density_weights: in place d = w != 0 ? 1/(a*w+b) : 0;
 *                         sums[0..2] = sum w, sum d*w, sum d*d*w over polarization 0
 *   `sums` are device float64 and are zeroed by the call.
 */
int kimg_grid_weights(float *grid, int64_t row_stride, int64_t pol_stride, int width, int height,
                      int num_polarizations, const int16_t *uv, const float *weights,
                      int64_t num_vis, void *stream);
int kimg_mean_weight(double *sums, const float *grid, int64_t row_stride, int width, int height,
                     void *stream);
int kimg_density_weights(double *sums, float *grid, int64_t row_stride, int64_t pol_stride,
                         int width, int height, int num_polarizations, float a, float b,
                         void *stream);
/* Robust weighting without the host between the two kernels (weight.py:525-531): a = robust /
 * (mean_sums[1] / mean_sums[0]) on the device, in the host's arithmetic (doubles, rounded to float32),
 * mean_sums = what kimg_mean_weight left on the DEVICE; robust = (5 * 10^-robustness)^2. */
int kimg_density_weights_robust(double *sums, float *grid, int64_t row_stride, int64_t pol_stride,
                                int width, int height, int num_polarizations,
                                const double *mean_sums, double robust, float b, void *stream);
/* UV taper and uv-range weighting fused into the density pass (CASA uvtaper / uvrange, WSClean
 * -taper-gaussian, -minuv-l, -maxuv-l, -taper-inner-tukey, -taper-edge-tukey).  The reference has
 * none; the semantics are this library's, and katsdpimager_amd/weight.py holds them once more as
 * numpy (uv_taper_host).  One kernel for natural (a = 0, b = 1), uniform (a = 1, b = 0) and robust
 * weighting: mean_sums NULL takes `a` as given, otherwise a = robust / (mean_sums[1] / mean_sums[0])
 * as in kimg_density_weights_robust and `a` is ignored.
 *
 * Cell (x, y) stands at u = (x - width / 2) * u_step, v = (y - height / 2) * v_step wavelengths
 * (the steps are 1 / image_size).  In float64, with r = sqrt(u u + v v):
 *   G = exp(-((quad_uu u u + quad_uv u v) + quad_vv v v))
 *   inner = 0 for r < min_uv; sin^2(pi/2 (r - min_uv) / inner_tukey) for r < min_uv + inner_tukey
 *           (inner_tukey > 0); else 1            [= 0.5 (1 - cos(pi x)), the raised cosine]
 *   outer = 0 for r > max_uv; sin^2(pi/2 (max_uv - r) / outer_tukey) for r > max_uv - outer_tukey
 *           (outer_tukey > 0); else 1
 *   t64 = G * inner * outer;  t = (float) t64, one rounding.
 * For an image-plane Gaussian of FWHM major, minor (l/m units) whose major axis stands at angle
 * theta from the m (v, row) axis towards the l (u, column) axis -- the angle beam.fit_beam reports --
 * and k = pi^2 / (4 ln 2), c = cos theta, s = sin theta:
 *   quad_uu = k (major^2 s^2 + minor^2 c^2), quad_uv = 2 k (major^2 - minor^2) s c,
 *   quad_vv = k (major^2 c^2 + minor^2 s^2).
 * No Gaussian: all three 0.  No cuts: min_uv = 0, max_uv = DBL_MAX (every field must be finite).
 * Per cell, for every polarization: d as kimg_density_weights computes it (the same float32
 * expression, 0 where w == 0); grid = d * t (float32 product).  Each stored value lies within
 * 3 * 2^-24 of d * t64 relatively where t is a normal float32, within 2^-126 absolutely otherwise.
 * sums over polarization 0: sums[0] = sum of w over the cells with t64 > 0 (a hard cut leaves the
 * sums the same data would give without the cut cells), sums[1] = sum e w, sums[2] = sum e e w with
 * e the stored float32.  The robust mean weight is the untapered one.
 * *taper is a HOST struct, read during the call and handed to the kernel by value.
 * KIMG_EINVAL, before anything is enqueued: a null pointer (mean_sums excepted), a non-finite or
 * negative field (quad_uv may be negative), a non-finite step or one that is not above 0,
 * row_pitch < width, an odd width or height.  (row_pitch, pol_pitch: the row and polarization
 * strides of kimg_density_weights, in elements; tests/test_uv_taper_gpu.py holds this call's
 * refusals, the row pitch below the width among them.) */
typedef struct kimg_uv_taper {
    double quad_uu, quad_uv, quad_vv;   /* the Gaussian's quadratic form, per wavelength^2 */
    double min_uv, max_uv;              /* cut radii, wavelengths */
    double inner_tukey, outer_tukey;    /* ramp widths, wavelengths */
} kimg_uv_taper;
int kimg_density_weights_taper(double *sums, float *grid, int64_t row_pitch, int64_t pol_pitch,
                               int width, int height, int num_polarizations, float a, float b,
                               const double *mean_sums, double robust, double u_step, double v_step,
                               const kimg_uv_taper *taper, void *stream);
int kimg_fill(float *data, int64_t count, float value, void *stream);

/* ---- visibility preprocessing: preprocess.cpp:390-513 (visibility_collector<P>::add_impl2) and
 * :334-372 (compress); the reference runs these on host cores (OpenMP) behind
 * preprocess.VisibilityCollector.add (preprocess.py:117-150).
 *   kimg_preprocess_convert: one channel, one buffer of num_vis inputs.  Per visibility: drop if any
 *       input weight is 0; xvis = M vis, xweights = 1/(|M|^2 (1/|w|)) with MulZ products; M =
 *       mueller_stokes [P][Q] when the feed angles are NULL, else mueller_stokes [P][4] x
 *       diag(RR, RL, conj RL, conj RR) x mueller_circular [4][Q] (:244-258); w<0 flip + conjugate;
 *       vis *= weight; non-finite -> 0; quantise (subpixel_coord :313-323, w :501-506).
 *       The two matrices are HOST pointers (interleaved re, im float32); everything else is device.
 *       Outputs: key int16 [N][6] = (u, v, sub_u, sub_v, w_plane, w_slice), out_weights float32 [N][P],
 *       out_vis complex64 [N][P]; dropped inputs give an all-zero record.
 *   kimg_preprocess_compress: skip records with weights[0] == 0, sum runs of adjacent equal keys
 *       left to right in float32, then order the results by w_slice keeping arrival order inside a
 *       slice.  Outputs are in the gridder's layout: out_uv int16 [M][4] = (u, v, sub_u, sub_v),
 *       out_w_plane int16 [M], out_weights [M][P], out_vis [M][P], and counts uint64 [w_slices]
 *       (device) = run length per slice, M = sum(counts).  Output arrays need room for N records.
 *       merge_window > 0: runs never cross a multiple of merge_window records -- the call then
 *       compresses num_vis / merge_window of the reference's buffers (preprocess.cpp:431-509: every
 *       buffer is compressed on its own) in ONE pass over the device, with the results the
 *       per-buffer calls would have given, concatenated per slice.  0 = one buffer.
 *       workspace: kimg_preprocess_workspace_bytes(N, P) bytes of device memory.
 *   kimg_real_to_complex: dst[i] = (src[i], 0): feeds weights as visibilities for the PSF pass
 *       (frontend.py:511) from a device-resident store.
 */
int kimg_preprocess_convert(int num_polarizations, int num_input_polarizations, int64_t num_vis,
                            const float *uvw, const float *weights, const void *vis,
                            const float *feed_angle1, const float *feed_angle2,
                            const float *mueller_stokes_host, const float *mueller_circular_host,
                            float max_w, int w_slices, int w_planes, int oversample, float cell_size,
                            int16_t *key, float *out_weights, void *out_vis, void *stream);
size_t kimg_preprocess_workspace_bytes(int64_t num_vis, int num_polarizations);
int kimg_preprocess_compress(int num_polarizations, int64_t num_vis, int w_slices,
                             const int16_t *key, const float *weights, const void *vis,
                             int16_t *out_uv, int16_t *out_w_plane, float *out_weights, void *out_vis,
                             uint64_t *counts, int64_t merge_window, void *workspace,
                             size_t workspace_bytes, void *stream);
int kimg_real_to_complex(void *dst, const float *src, int64_t count, void *stream);

/* ---- once-per-channel re-ordering of a stored W-slice (csrc/store.hip).  No launch site of the
 * reference corresponds to it: the reference's preprocessor leaves a slice in arrival order
 * (baseline-sorted load blocks, adjacent-merged: loader_ms.py:465-468, preprocess.cpp:334-397) and
 * its gridder bins per pass inside the kernel (grid.mako; grid.py:436-463 get_bin_size).  The
 * resident store (preprocess.VisibilityCollectorDevice) calls this once when it is closed; every
 * later pass of the channel runs the window kernels on the result.
 *   order: strips of (32 - taps + 1) grid columns (taps = kernel_width, or (kernel_width + 1) / 2
 *       for widths above 32), each strip sorted by v, odd strips backwards; stable.
 *   merge != 0: the sort also covers (u in strip, sub_v, sub_u, w_plane), and every run of records
 *       with equal (u, v, sub_u, sub_v, w_plane) becomes ONE record whose weights and visibilities
 *       are the run's sums, added left to right in float32 in arrival order -- compress() of
 *       preprocess.cpp:334-372 applied to whole-slice runs instead of arrival runs.
 *   Outputs need room for num_vis records; *out_count (device uint64) = records written.
 *   workspace: kimg_store_reorder_workspace_bytes(num_vis) bytes (28 per record + sort scratch). */
size_t kimg_store_reorder_workspace_bytes(int64_t num_vis);
int kimg_store_reorder(int num_polarizations, int64_t num_vis, int kernel_width, int oversample,
                       int w_planes, int merge, const int16_t *uv, const int16_t *w_plane,
                       const float *weights, const void *vis, int16_t *out_uv, int16_t *out_w_plane,
                       float *out_weights, void *out_vis, uint64_t *out_count, void *workspace,
                       size_t workspace_bytes, void *stream);

/* ---- grid <-> image: image.py:649-673 GridToImage._run, :716-740 ImageToGrid._run,
 * :153-180 _LayerImage._run + layer_to_image.mako / image_to_layer.mako.
 *   kimg_grid_to_layer: zero the GxG layer and copy the centred Gg x Gg grid of one
 *       polarization into its corners (DC at [0][0]) -- the reference's zero + 4 copy_region.
 *   kimg_layer_to_grid: the inverse copy (corners -> centred grid).
 *   kimg_layer_to_image: image[pol] += Re(layer * e^{2 pi i w (n-1)}) * n / (k1d[y] k1d[x]),
 *       with fftshift; l = x*lm_scale + lm_bias.  layer is row-contiguous GxG.
 *   kimg_image_to_layer: layer = image[pol] / (k1d[y] k1d[x] n) * e^{-2 pi i w (n-1)}.
 */
int kimg_grid_to_layer(void *layer, int layer_size, const void *grid, int64_t grid_row_stride,
                       int grid_size, void *stream);
int kimg_layer_to_grid(void *grid, int64_t grid_row_stride, int grid_size, const void *layer,
                       int layer_size, void *stream);
int kimg_layer_to_image(float *image, int64_t image_row_stride, const void *layer, int size,
                        const float *kernel1d, float lm_scale, float lm_bias, float w,
                        void *stream);
int kimg_image_to_layer(void *layer, const float *image, int64_t image_row_stride, int size,
                        const float *kernel1d, float lm_scale, float lm_bias, float w,
                        void *stream);
/* The float64 forms of the four calls above: complex128 grid and layer, float64 image and kernel1d,
 * double lm_scale / lm_bias / w; the phase from double sincospi.  Float64 takes this plain route
 * (copy, kimg_fft_plan_create_f64 transform, layer -> image) for every w. */
int kimg_grid_to_layer_f64(void *layer, int layer_size, const void *grid, int64_t grid_row_stride,
                           int grid_size, void *stream);
int kimg_layer_to_grid_f64(void *grid, int64_t grid_row_stride, int grid_size, const void *layer,
                           int layer_size, void *stream);
int kimg_layer_to_image_f64(double *image, int64_t image_row_stride, const void *layer, int size,
                            const double *kernel1d, double lm_scale, double lm_bias, double w,
                            void *stream);
int kimg_image_to_layer_f64(void *layer, const double *image, int64_t image_row_stride, int size,
                            const double *kernel1d, double lm_scale, double lm_bias, double w,
                            void *stream);
/* The same pair for a layer whose transform is only wanted for its real part, i.e. w = 0 (the
 * phase factor of layer_to_image is then exactly 1): the reference notes at image.py:561-566 that a
 * complex-to-real transform would do; here it does.
 *   kimg_grid_to_half_layer: half_layer[ly][lx], lx = 0 .. G/2 (rows of G/2 + 1 complex values),
 *       = (g(k) + conj g(-k)) / 2 of the zero-padded, corner-DC layer g that kimg_grid_to_layer
 *       would have made: the Hermitian part of g, whose inverse transform is Re F^-1[g].
 *   kimg_real_layer_to_image: image[pol] += layer * n / (k1d[y] k1d[x]) with fftshift, from the REAL
 *       output of kimg_rfft_exec(direction +1); layer_row_stride in floats (G + 2 when the
 *       transform ran in place on the half layer). */
int kimg_grid_to_half_layer(void *half_layer, int layer_size, const void *grid,
                            int64_t grid_row_stride, int grid_size, void *stream);
int kimg_real_layer_to_image(float *image, int64_t image_row_stride, const float *layer,
                             int64_t layer_row_stride, int size, const float *kernel1d,
                             float lm_scale, float lm_bias, void *stream);
/* ... and the other way (ImageToGrid, image.py:676-740) at w = 0, where the layer is real:
 *   kimg_image_to_real_layer: layer = image[pol] / (k1d[y] k1d[x] n) with fftshift, rows of
 *       layer_row_stride floats (G + 2 for the in-place real-to-complex kimg_rfft_exec, direction -1);
 *   kimg_half_layer_to_grid: the centred grid from the half spectrum [G][G/2 + 1] that transform
 *       leaves, F(-k) = conj F(k) for the columns it does not hold. */
int kimg_image_to_real_layer(float *layer, int64_t layer_row_stride, const float *image,
                             int64_t image_row_stride, int size, const float *kernel1d,
                             float lm_scale, float lm_bias, void *stream);
int kimg_half_layer_to_grid(void *grid, int64_t grid_row_stride, int grid_size,
                            const void *half_layer, int layer_size, void *stream);
/* The whole of GridToImage.__call__ / ImageToGrid.__call__ (image.py:609-673, :676-740) for one
 * polarization at w = 0 in two launches, with transforms of the library's own (even layer sizes
 * 16 .. 8192 with no prime factor above 7 -- every size parameters.py:17-25 of the reference picks
 * in that range; mixed radix 4 / 2 / 3 / 5 / 7 in LDS): only the Gg/2 + 1 columns of the half layer the grid reaches
 * are transformed, the fold / padding and the image correction are the prologue and epilogue of
 * the transform kernels, and what passes between the two launches is (Gg/2 + 1) x G cells in
 * `workspace` (16-byte aligned, kimg_grid_image_real_workspace_bytes; the layer buffer will do).
 * Results equal the route above up to the rounding of the transform.  accumulate = 0: the image
 * is written, not added to (what the reference gets by zeroing it first, imaging.py:258-261:
 * saves the fill and the read).
 *   kimg_grid_image_real_supported: 1 when the two functions take these sizes, else 0.
 *
 * Arithmetic the five functions below promise (tests/test_transform_truth.py restates it).  fl()
 * is one float32 rounding; nothing is fused except where fma() is written (the library is built
 * with -ffp-contract=off); sqrt and / are correctly rounded (hipcc's default for float32 when no
 * fast-math flag is given; katsdpimager_amd/build.py FLAGS gives none and must not).  G = layer_size, Gg = grid_size, h = Gg / 2; image index y <-> layer index
 * sy = (y + G/2) mod G; grid index gy <-> frequency cy = gy - h <-> layer index cy mod G.
 *   l(x)   = fl(fl((float) x * lm_scale) + lm_bias), m(y) likewise;
 *   n(y,x) = sqrt(fl(1 - fl(fl(m m) + fl(l l))))      (lm_scale = 0, lm_bias = 0 is taken: n = 1);
 *   p(y,x) = fl(w * fl(n - 1)) turns, r = p - rint(p) (exact), c + i s = cospi(2 r) + i sinpi(2 r);
 *            the image -> grid direction uses fl(-w * fl(n - 1)) = -p, so c - i s;
 *   t(y,x) = fl(k[y] * k[x]) with k = kernel1d.
 * The transforms F are unnormalised sums of G terms per axis, sign + grid -> image and - image ->
 * grid, evaluated in float32 as decimation-in-time stages of radix 4 (as many as fit), 2 (at most
 * one), 3, 5, 7 in that order; a complex product a b is (fma(a.x, b.x, -fl(a.y b.y)),
 * fma(a.x, b.y, fl(a.y b.x))); the twiddles e^{2 pi i j / (r q)} of a stage are double values rounded to
 * float32, their powers float32 products of those, the 3rd, 5th and 7th roots of unity float32
 * constants.  The order of the sums inside F is not part of the contract; its accuracy is (the
 * test module's bound).
 *   grid -> image, w = 0: the layer is the grid's Hermitian part, fl(0.5 (g(c) + conj g(-c))) per
 *     component, with g = 0 outside -h .. h - 1 (so row and column -h meet no partner unless
 *     Gg = G, where -G/2 is its own mirror); v = Re F;
 *     out = fl(fl(v n) / t); image = out (accumulate = 0) or fl(image + out).
 *   grid -> image, any w: v = fl(fl(Re F c) - fl(Im F s)); out and image as above.  At w = 0 this
 *     is the same quantity as the function above, by another sum.
 *   image -> grid, w = 0: layer = fl(image / fl(t n)); grid cell (gy, gx) = F at (cy, cx).  Every
 *     cell of the Gg x Gg grid is overwritten, nothing is added to it; cells of a row beyond
 *     grid_size (grid_row_stride) are not touched.
 *   image -> grid, any w: u = fl(image / fl(t n)), layer = (fl(u c), -fl(u s)); grid as above.
 *   kimg_convolve_beam: per cell (v, u) of the half spectrum, v = ly - size if 2 ly >= size else
 *     ly, u = 0 .. size/2: power = fl(fl(fl(fl(a v) + fl(b u)) v) + fl(fl(c u) u)), factor =
 *     fl(amplitude * expf(power)), spectrum cell times factor per component; rows forward, columns
 *     forward, factor, columns inverse, rows inverse.  Nothing is divided by size^2: the caller
 *     folds it into `amplitude`.
 * Every function writes `workspace` only below the byte count its _workspace_bytes function
 * returns, refuses (KIMG_EINVAL, nothing written) a workspace that is smaller or not 16-byte
 * aligned, a stride below the width and sizes kimg_grid_image_real_supported refuses, and leaves
 * the cells of a row beyond the width alone. */
int kimg_grid_image_real_supported(int layer_size, int grid_size);
size_t kimg_grid_image_real_workspace_bytes(int layer_size, int grid_size);
int kimg_grid_to_image_real(float *image, int64_t image_row_stride, int layer_size,
                            const void *grid, int64_t grid_row_stride, int grid_size,
                            const float *kernel1d, float lm_scale, float lm_bias, int accumulate,
                            void *workspace, size_t workspace_bytes, void *stream);
int kimg_image_to_grid_real(void *grid, int64_t grid_row_stride, int grid_size,
                            const float *image, int64_t image_row_stride, int layer_size,
                            const float *kernel1d, float lm_scale, float lm_bias,
                            void *workspace, size_t workspace_bytes, void *stream);
/* ... and for any w (a slice of the W stack away from w = 0: the layer is complex, image.py:781-799
 * and :836-848 with the phase e^{+-2 pi i w (n - 1)}): the same two launches over the Gg columns the
 * grid reaches and over pairs of rows, each row with a complex transform of its own.  Same sizes as
 * the w = 0 pair (kimg_grid_image_real_supported); workspace Gg x G cells. */
size_t kimg_grid_image_w_workspace_bytes(int layer_size, int grid_size);
int kimg_grid_to_image_w(float *image, int64_t image_row_stride, int layer_size,
                         const void *grid, int64_t grid_row_stride, int grid_size,
                         const float *kernel1d, float lm_scale, float lm_bias, float w,
                         int accumulate, void *workspace, size_t workspace_bytes, void *stream);
int kimg_image_to_grid_w(void *grid, int64_t grid_row_stride, int grid_size,
                         const float *image, int64_t image_row_stride, int layer_size,
                         const float *kernel1d, float lm_scale, float lm_bias, float w,
                         void *workspace, size_t workspace_bytes, void *stream);

/* ConvolveBeam.__call__ (beam.py:351-398) for a square image of a size the functions above take
 * (kimg_grid_image_real_supported(size, size)), in three launches on the library's own transforms:
 * rows (two real rows per complex transform) -> per column of the half spectrum: forward transform,
 * times amplitude * exp((a v + b u) v + c u^2) (kimg_fourier_beam's factor; 1 / (H W) folded into
 * the amplitude as there), inverse transform -> rows back.  In place on `image`; workspace =
 * (size / 2 + 1) x size cells, 16-byte aligned (the operator's `fourier` buffer). */
int kimg_convolve_beam(float *image, int64_t row_stride, int size, float amplitude, float a,
                       float b, float c, void *workspace, size_t workspace_bytes, void *stream);

/* 2-D complex-to-complex FFT plans (katsdpsigproc.fft.FftTemplate, image.py:585-600,629,698)
 * on rocFFT (called directly); unnormalised, in place.  direction: -1 forward, +1 inverse. */
int kimg_fft_plan_create(void **plan, int size_y, int size_x);
/* The same for complex128 layers (rocfft_precision_double); exec and destroy take either kind. */
int kimg_fft_plan_create_f64(void **plan, int size_y, int size_x);
int kimg_fft_exec(void *plan, void *layer, int direction, void *stream);
int kimg_fft_plan_destroy(void *plan);

/* Restoring-beam convolution (beam.py:204-398: FourierBeam._run :283-311 + fourier_beam.mako,
 * ConvolveBeam :351-398 = R2C FFT, multiply, C2R FFT), one polarization plane at a time.
 *   kimg_rfft_*: out-of-place real <-> half-complex 2-D plans; image float32 [H][W] dense,
 *       fourier complex64 [H][W/2+1] dense; direction -1 = R2C forward, +1 = C2R inverse
 *       (unnormalised; the C2R transform overwrites `fourier`).
 *   kimg_fourier_beam: data[y][x] *= amplitude * exp((a v + b u) v + c u u), u = x,
 *       v = y < H/2 ? y : y - H  (the caller folds 1/(H W) and the axis scaling into
 *       amplitude, a, b, c exactly as beam.py:287-299).  width = W/2+1 columns. */
int kimg_rfft_plan_create(void **plan, int height, int width);
int kimg_rfft_exec(void *plan, float *image, void *fourier, int direction, void *stream);
int kimg_rfft_plan_destroy(void *plan);
int kimg_fourier_beam(void *data, int64_t row_stride, int width, int height, float amplitude,
                      float a, float b, float c, void *stream);

/* ---- image-plane streams: image.py:351-367, :439-458, :539-558 (+ scale.mako,
 * add_image.mako, apply_primary_beam.mako).  scale_host: P floats on the HOST. */
int kimg_scale(float *image, int64_t row_stride, int64_t pol_stride, int width, int height,
               int num_polarizations, const float *scale_host, void *stream);
/* The scaling of frontend.py:541-545 (dirty and PSF by 1 / the PSF's central pixel) without the host in
 * between: out[p] = 1 / image[p][y][x] on the device (np.reciprocal of a float32), and kimg_scale with
 * its factors read from device memory.  scale, out: P floats on the DEVICE. */
int kimg_pixel_reciprocal(const float *image, int64_t row_stride, int64_t pol_stride, int width,
                          int height, int num_polarizations, int x, int y, float *out, void *stream);
int kimg_scale_device(float *image, int64_t row_stride, int64_t pol_stride, int width, int height,
                      int num_polarizations, const float *scale, void *stream);
int kimg_add_image(float *dest, int64_t dest_row_stride, int64_t dest_pol_stride,
                   const float *src, int64_t src_row_stride, int64_t src_pol_stride,
                   int width, int height, int num_polarizations, void *stream);
int kimg_apply_primary_beam(float *image, int64_t row_stride, int64_t pol_stride,
                            const float *beam_power, int64_t beam_row_stride,
                            int width, int height, int num_polarizations,
                            float threshold, float replacement, void *stream);
/* The float64 forms of kimg_scale, kimg_add_image and kimg_apply_primary_beam (float64 images and
 * beam; scale_host: P doubles on the HOST). */
int kimg_scale_f64(double *image, int64_t row_stride, int64_t pol_stride, int width, int height,
                   int num_polarizations, const double *scale_host, void *stream);
int kimg_add_image_f64(double *dest, int64_t dest_row_stride, int64_t dest_pol_stride,
                       const double *src, int64_t src_row_stride, int64_t src_pol_stride,
                       int width, int height, int num_polarizations, void *stream);
int kimg_apply_primary_beam_f64(double *image, int64_t row_stride, int64_t pol_stride,
                                const double *beam_power, int64_t beam_row_stride,
                                int width, int height, int num_polarizations,
                                double threshold, double replacement, void *stream);

/* Output statistics of the restore step (frontend.py:171-209, host loops in the reference):
 *   kimg_image_peak:   find_peak -- max |image| over all polarizations and pixels with
 *       |image| * pbeam[y][x] > 7.5 * noise (pbeam float32 [H][W], may be NULL = 1; NaNs never
 *       pass).  *peak (device float32) receives the maximum, 0 when no pixel qualifies (the
 *       reference returns NaN then; the host wrapper does the same).
 *   kimg_image_nansum: get_totals -- sums[p] (device float64 [P], zeroed by the call) = sum of
 *       the non-NaN pixels of polarization p. */
int kimg_image_peak(const float *image, int64_t row_stride, int64_t pol_stride, const float *pbeam,
                    int64_t beam_row_stride, int width, int height, int num_polarizations,
                    float noise, float *peak, void *stream);
int kimg_image_nansum(const float *image, int64_t row_stride, int64_t pol_stride, int width,
                      int height, int num_polarizations, double *sums, void *stream);

/* ---- CLEAN support: clean.py:123-163 PsfPatch.__call__ + psf_patch.mako
 * bound (device int32[2], zeroed by the call) receives max |x-mid_x|, max |y-mid_y| over
 * pixels in [min_x,max_x]x[min_y,max_y] where any polarization has |psf| >= threshold. */
int kimg_psf_patch(const float *psf, int64_t row_stride, int64_t pol_stride, int num_polarizations,
                   int min_x, int min_y, int max_x, int max_y, int mid_x, int mid_y,
                   float threshold, int32_t *bound, void *stream);

/* Noise estimate support (clean.py:295-353 NoiseEst.__call__ + rank.mako, host semantics of
 * clean.py:938-943): one radix-select pass.  hist (device uint32[256], zeroed by the call)
 * receives the histogram of byte `pass` (3 = most significant) of the bit pattern of |x| over
 * the region inside `border`, restricted to values whose higher bytes equal `prefix`. */
int kimg_abs_histogram(const float *image, int64_t row_stride, int64_t pol_stride,
                       int width, int height, int num_polarizations, int border,
                       int pass, uint32_t prefix, uint32_t *hist, void *stream);
/* out[0] = count of |x| <= value, out[1] = bit pattern of min |x| > value (0xFFFFFFFF if none);
 * out is device uint32[2], initialised by the call. */
int kimg_abs_count_le(const float *image, int64_t row_stride, int64_t pol_stride,
                      int width, int height, int num_polarizations, int border,
                      float value, uint32_t *out, void *stream);

/* ---- CLEAN minor cycle: clean.py:451-480 _UpdateTiles.__call__, :566-587 _FindPeak._run,
 * :683-726 _SubtractPsf.__call__ (+ update_tiles.mako, find_peak.mako, subtract_psf.mako).
 * Tie-breaks follow the reference HOST path bit-exactly: first strict maximum in row-major
 * order within a tile (clean.py:953-958), first maximum tile in row-major order
 * (np.argmax, clean.py:1062).
 *   dirty/model/psf float32 [P][height][width]; tile_max float32 [tiles_y][tiles_x];
 *   tile_pos int32 [tiles_y][tiles_x][2] = (y, x); tiles are 32x32 starting at `border`.
 */
int kimg_update_tiles(const float *dirty, int64_t row_stride, int64_t pol_stride,
                      int width, int height, int num_polarizations, int border, int mode,
                      float *tile_max, int32_t *tile_pos, int tiles_x, int tiles_y,
                      int tile_x0, int tile_y0, int tile_x1, int tile_y1, void *stream);
int kimg_find_peak(const float *dirty, int64_t row_stride, int64_t pol_stride,
                   int num_polarizations, const float *tile_max, const int32_t *tile_pos,
                   int tiles_x, int tiles_y,
                   float *peak_value, int32_t *peak_pos, float *peak_pixel, void *stream);
int kimg_subtract_psf(float *dirty, float *model, int64_t row_stride, int64_t pol_stride,
                      int width, int height, int num_polarizations,
                      const float *psf, int64_t psf_row_stride, int64_t psf_pol_stride,
                      int psf_width, int psf_height, int patch_width, int patch_height,
                      const float *peak_pixel, int pos_x, int pos_y, float loop_gain,
                      void *stream);

/* The whole noise estimate of NoiseEst.__call__ / noise_est_host (clean.py:305-353, :938-943) without
 * host round trips: four radix-select passes with the byte chosen on the device, the counting pass
 * when the number of samples is even, then out[0] = median(|x| inside the border) * median_to_rms
 * (float32 arithmetic as numpy's: (lo + hi) / 2 * scale).  scratch: kimg_noise_est_scratch_bytes()
 * bytes of device memory, initialised by the call; out: device float32[1]. */
size_t kimg_noise_est_scratch_bytes(void);
int kimg_noise_est(const float *image, int64_t row_stride, int64_t pol_stride,
                   int width, int height, int num_polarizations, int border,
                   float median_to_rms, void *scratch, float *out, void *stream);

/* Device-resident minor-cycle loop (replaces the per-cycle host round trip of
 * clean.py:848-891): runs up to `max_cycles` cycles of find-peak -> threshold test ->
 * subtract -> tile update without host synchronisation.
 *   state  device scratch, kimg_clean_state_bytes(P, tiles_x, tiles_y) bytes, initialised by the
 *          call (loop state, and for the one-launch-per-cycle form used with small PSF patches
 *          the per-tile peak pixel values and the tile records in flight between cycles)
 *   log    device float32 [max_cycles][3 + P]: (metric, y, x as float bits, loop_gain*pixel[p])
 *   form   KIMG_CLEAN_FORM_*
 *   After the stream is synchronised, ((int32*)state)[0] holds the number of cycles done
 *   (stops early when the peak metric < threshold, clean.py:879-880).
 */
size_t kimg_clean_state_bytes(int num_polarizations, int tiles_x, int tiles_y);
int kimg_clean_cycles(float *dirty, float *model, int64_t row_stride, int64_t pol_stride,
                      int width, int height, int num_polarizations,
                      const float *psf, int64_t psf_row_stride, int64_t psf_pol_stride,
                      int psf_width, int psf_height, int patch_width, int patch_height,
                      int border, int mode, float loop_gain, float threshold,
                      float *tile_max, int32_t *tile_pos, int tiles_x, int tiles_y,
                      int max_cycles, int form, void *state, float *log, void *stream);

/* The minor cycles of ONE MAJOR CYCLE in one call (the loop of frontend.py:560-585): the first cycle
 * runs without a threshold (clean.py:879: its component is always taken); the rest stop below
 *     max(noise_threshold, left_for_next * power of the first peak)      (frontend.py:568-575)
 * -- or do not run at all if the first peak itself is not above that -- worked out on the device in
 * the host's arithmetic (doubles; a metric as a flux and back as clean.py:166-184 has it), so that the
 * host round trip between the first cycle and the others is gone.  On every route -- this call, or
 * a host that makes the threshold itself and passes it to kimg_clean_cycles and its kin -- the
 * threshold is that float64 expression rounded ONCE to the float32 the metrics are compared with
 * (a cycle stops at metric < threshold); the float32 peak and noise estimate enter it as doubles.
 * Arguments as kimg_clean_cycles;
 * noise_threshold = noise estimate x the clean threshold (in sigma), left_for_next = 1 - major gain;
 * max_cycles counts the first cycle.  The log's first row is the first cycle's.  Runs where the
 * multi-component form does (form: KIMG_CLEAN_FORM_AUTO or _MULTI with its caps); KIMG_EUNSUPPORTED
 * otherwise, and the caller takes the two steps of the reference.
 * cycles_done, first_peak (host pointers, either may be null): the number of cycles done and the
 * metric of the first one, which the call has from the words the device writes for it -- what a
 * driver needs to decide on the next major cycle without reading the device back (state and log can
 * then be fetched while the next stage runs). */
int kimg_clean_major_cycles(float *dirty, float *model, int64_t row_stride, int64_t pol_stride,
                            int width, int height, int num_polarizations,
                            const float *psf, int64_t psf_row_stride, int64_t psf_pol_stride,
                            int psf_width, int psf_height, int patch_width, int patch_height,
                            int border, int mode, float loop_gain, double noise_threshold,
                            double left_for_next, float *tile_max, int32_t *tile_pos, int tiles_x,
                            int tiles_y, int max_cycles, int form, void *state, float *log, void *stream,
                            int *cycles_done, float *first_peak);

/* The same loop for several channels of a band at once: cycle i of every channel runs in ONE
 * launch (the reference loops over channels serially, frontend.py:749-767, and within a channel
 * over cycles with a host round trip each, clean.py:848-891).  A minor cycle is a latency chain
 * that occupies a fraction of the device; the channels' images have the same shape, so their
 * cycles share the kernel boundary.  Each channel keeps its own images, PSF and patch size, tile
 * arrays, state / log buffers (as for kimg_clean_cycles), threshold and cycle limit, and stops on
 * its own; the results per channel are bit-identical to kimg_clean_cycles on that channel alone.
 *   channels_host  HOST array of num_channels (<= KIMG_CLEAN_BATCH_MAX) descriptors; the device
 *                  pointers in them follow the conventions of kimg_clean_cycles
 *   Every channel's patch must allow the one-launch-per-cycle form (at most 32 x 32 lattice
 *   blocks and (patch_width / 32 + 2) * (patch_height / 32 + 3) <= 256): KIMG_EUNSUPPORTED
 *   otherwise, and the caller runs the channels one by one. */
#define KIMG_CLEAN_BATCH_MAX 8
typedef struct kimg_clean_channel {
    float *dirty, *model;
    const float *psf;
    float *tile_max;
    int32_t *tile_pos;
    void *state;
    float *log;
    int32_t patch_width, patch_height;
    float threshold;
    int32_t max_cycles;
} kimg_clean_channel;
int kimg_clean_cycles_batch(const kimg_clean_channel *channels_host, int num_channels,
                            int64_t row_stride, int64_t pol_stride, int width, int height,
                            int num_polarizations, int64_t psf_row_stride, int64_t psf_pol_stride,
                            int psf_width, int psf_height, int border, int mode, float loop_gain,
                            int tiles_x, int tiles_y, void *stream);

/* ---- CLEAN masks (clean windows): a per-pixel allow map for the minor cycle.  The reference has
 * none; the semantics are this library's.
 *   mask   device uint8 [height][width] with mask_row_stride bytes between rows (>= width); ONE
 *          plane serves all polarizations; nonzero = a component may be placed on this pixel.
 *   Candidates.  A pixel is a candidate only if it is inside the border AND allowed; the metric of
 *          every other pixel takes no part in any tile maximum.
 *   Subtraction is unchanged: the whole PSF patch is subtracted around a component, masked pixels
 *          included.  Only allowed pixels ever receive flux in the model.
 *   Scan order and tie-breaks are those of the unmasked calls: first strict maximum in row-major
 *          order within a tile, then the first maximal tile in row-major tile order.
 *   Empty tiles.  A tile without a candidate (or whose candidates all have metric 0) records
 *          tile_max = 0 and the tile_pos an all-zero tile records without a mask.
 *   Stopping.  With a mask, a best metric of exactly 0 ends the search whatever the threshold, 0
 *          included (otherwise an all-masked field would place a component on a masked pixel
 *          through the start position an empty tile records): kimg_find_peak_masked then writes
 *          peak_value 0, peak_pos (-1, -1) and a zero peak_pixel; kimg_clean_cycles_masked stops
 *          and logs nothing for that cycle.  Unmasked calls keep their behaviour at metric 0.
 * Each call takes the arguments of its unmasked namesake plus the mask.  A NULL mask means
 * unmasked: the call then runs exactly what the namesake runs.
 * kimg_clean_cycles_masked with a mask runs KIMG_CLEAN_FORM_TWO_LAUNCH or _ONE_LAUNCH (the latter
 * with its fallback); _AUTO chooses between these two; _MULTI, _PERSISTENT and _ONE_WORKGROUP asked
 * for with a mask return KIMG_EUNSUPPORTED before anything is enqueued.  kimg_clean_major_cycles and
 * kimg_clean_cycles_batch have no masked form. */
int kimg_update_tiles_masked(const float *dirty, int64_t row_stride, int64_t pol_stride,
                             int width, int height, int num_polarizations, int border, int mode,
                             float *tile_max, int32_t *tile_pos, int tiles_x, int tiles_y,
                             int tile_x0, int tile_y0, int tile_x1, int tile_y1, void *stream,
                             const uint8_t *mask, int64_t mask_row_stride);
int kimg_find_peak_masked(const float *dirty, int64_t row_stride, int64_t pol_stride,
                          int num_polarizations, const float *tile_max, const int32_t *tile_pos,
                          int tiles_x, int tiles_y,
                          float *peak_value, int32_t *peak_pos, float *peak_pixel, void *stream,
                          const uint8_t *mask, int64_t mask_row_stride);
int kimg_clean_cycles_masked(float *dirty, float *model, int64_t row_stride, int64_t pol_stride,
                             int width, int height, int num_polarizations,
                             const float *psf, int64_t psf_row_stride, int64_t psf_pol_stride,
                             int psf_width, int psf_height, int patch_width, int patch_height,
                             int border, int mode, float loop_gain, float threshold,
                             float *tile_max, int32_t *tile_pos, int tiles_x, int tiles_y,
                             int max_cycles, int form, void *state, float *log, void *stream,
                             const uint8_t *mask, int64_t mask_row_stride);

/* ---- CLEAN auto-masks: a clean mask built on the device from the residual image.  Masks have the
 * layout of "CLEAN masks": uint8 [height][width] with a row pitch in bytes (>= width), one plane
 * for all polarizations, nonzero = allowed.  Every byte these calls write is exactly 0 or 1; bytes
 * of the row padding (x >= width) are never written.  A pitch is what the other calls name a
 * stride: the distance between rows (or polarization planes), in elements of the array, at least
 * the width (KIMG_EINVAL otherwise, before anything is enqueued).  Pitches and widths are arbitrary.
 *
 * kimg_mask_threshold: mask[y][x] = 1 where the pixel is inside the border (border <= x < width -
 *   border, the same for y; a border of half the image or more leaves no such pixel) and
 *   metric(y, x) > threshold, else 0.  metric is the CLEAN metric of `mode`: |pol 0| for
 *   KIMG_CLEAN_I, the sum of squares over the polarizations, in polarization order and every
 *   operation rounded on its own, for KIMG_CLEAN_SUMSQ.  The comparison is strict: threshold 0
 *   selects the pixels with a nonzero metric, a negative threshold every pixel inside the border, a
 *   NaN metric or a NaN threshold nothing.  num_polarizations is 1 to 4.
 *
 * kimg_mask_dilate: out = ((in (+) disk(radius)) | or_with) & and_with, where (+) is the dilation
 *   by the Euclidean disk {(dy, dx): dy^2 + dx^2 <= radius^2} (integers), clipped at the edges of
 *   the plane: out is set where a nonzero byte of `in` lies within the disk around the pixel.
 *   radius is 0 to KIMG_MASK_MAX_RADIUS; radius 0 is a copy (to 0 / 1) followed by the combination.
 *   A NULL or_with or and_with drops that term; nonzero bytes of either count as set.
 *   count, if not NULL, receives the number of set pixels of `out` (device uint32; the call zeroes
 *   it on the stream, the kernel adds to it once per workgroup).
 *   Aliasing: or_with may be `out` itself (every byte is read before it is written, by the same
 *   thread: a cumulative mask).  `in` and and_with must not overlap `out`; in == out and
 *   and_with == out are KIMG_EINVAL before anything is enqueued.
 *   The cost per pixel is linear in the radius. */
#define KIMG_MASK_MAX_RADIUS 64
int kimg_mask_threshold(const float *image, int64_t row_pitch, int64_t pol_pitch,
                        int width, int height, int num_polarizations, int border, int mode,
                        float threshold, uint8_t *mask, int64_t mask_row_pitch, void *stream);
int kimg_mask_dilate(const uint8_t *in, int64_t in_row_pitch, uint8_t *out,
                     int64_t out_row_pitch, int width, int height, int radius,
                     const uint8_t *or_with, int64_t or_row_pitch,
                     const uint8_t *and_with, int64_t and_row_pitch, uint32_t *count,
                     void *stream);

/* ---- Multi-scale CLEAN: Gaussian scales beside the Hogbom minor cycle (clean_scales.hip).  The
 * reference has none; the semantics are this library's, and katsdpimager_amd/multiscale.py holds
 * them once more as numpy (MultiScaleCleanHost), which the device matches bit for bit.  float32,
 * KIMG_CLEAN_I only.  Every a * b + c below is a rounded multiply and then a rounded add.
 *
 * Scales.  Scale k has a radius R_k (0 .. KIMG_CLEAN_SCALES_MAX_RADIUS, R_0 = 0) and 2 R_k + 1
 *   taps t_k (scale 0: the single tap 1).  The caller makes the taps (float64, normalised to sum
 *   1, rounded once) and, for every pair j <= k, the cross taps t_jk of radius R_j + R_k (the
 *   float64 convolution of the unrounded t_j and t_k, rounded once).  At most
 *   KIMG_CLEAN_SCALES_MAX scales.  More scales or a larger radius: KIMG_EUNSUPPORTED.
 * conv(img, t), kimg_image_convolve_separable: a horizontal pass from `in` into `tmp`, then a
 *   vertical pass from `tmp` into `out`; each pass is acc = 0, then acc = acc + t[i] * in[c - R + i]
 *   for i = 0 .. 2 R in this order, taps that fall outside the image skipped; every polarization
 *   plane on its own.  taps: DEVICE float [2 R + 1].  `out` may be `in`; `tmp` is neither.  Bytes
 *   of the row padding are never written.
 * Set-up.  n_k = conv(psf, t_kk)[0][centre][centre], inv_k = 1.0f / n_k.  The residual of scale k
 *   is conv(dirty, t_k) * inv_k for k >= 1 and the dirty image ITSELF for k = 0: the PSF's central
 *   pixel (polarization 0) must be exactly 1 (KIMG_EINVAL otherwise; the set-up reads it back).
 *   The cross patch X_jk = crop(conv(psf, t_jk)) * inv_j, the crop being the centred box of
 *   (patch + 2 (R_j + R_k)) pixels a side -- from centre - size / 2, as the Hogbom calls place the
 *   patch -- clipped to the image.  The PSF has the image's width and height.
 *   what: KIMG_CLEAN_SCALES_PSF (taps, n, inv, X: once per PSF) | KIMG_CLEAN_SCALES_RESIDUALS (the
 *   residuals of the scales k >= 1 from the dirty image as it stands, and every tile record; with
 *   `mask` only allowed pixels are candidates, as under "CLEAN masks").
 *   taps_host: HOST float [num_scales][192], cross_taps_host: HOST float [pairs][320], the pairs
 *   (j, k), j <= k, in row-major order; rows are padded with anything.
 * A cycle.  Peak of every scale from its tile records (the Hogbom tile structure over |residual of
 *   polarization 0|); the scale k* with the largest biases[k] * peak_k (a float32 product; ties to
 *   the smallest k); stop if the unbiased peak < threshold, or, with a mask, if it is 0;
 *   a[p] = loop_gain * residual_k*[p][pos]; for every scale j, residual_j[p] -= a[p] * X_j,k*[p]
 *   over the box of X_j,k* centred on pos, clipped to the image (and to what X holds);
 *   model[p] += a[p] * (t_k*[dy] * t_k*[dx]) over the (2 R_k* + 1)^2 box, clipped; the touched
 *   tiles of every scale rescanned.  Log row: (k*, y, x as int32 bit patterns, peak, a[0 .. P-1]),
 *   4 + P floats; log holds max_cycles rows.
 *   kimg_clean_scales_cycles runs up to max_cycles cycles with plain launches, in chunks of 64; it
 *   reads the device's `done` word between chunks (a stream synchronisation per chunk, none per
 *   component) and returns with the stream idle and *cycles_done set.  model has the dirty image's
 *   pitches.  radii, biases: HOST arrays [num_scales].  mode KIMG_CLEAN_SUMSQ: KIMG_EUNSUPPORTED.
 * Workspace (16-byte aligned; KIMG_EWORKSPACE if too small): sections in this order, each a multiple
 *   of 64 floats: state 64 | n at 0 and inv at 8 of 64 | taps 6 * 192 | cross taps 21 * 320 rounded
 *   up | tile_max [K][T'] | tile_pos [K][T'][2] int32, T' = tiles_x * tiles_y rounded up |
 *   residuals k = 1 .. K-1, each [P][height][width] dense, rounded up | X_jk for j, k row-major,
 *   each [P][crop height][crop width] dense, rounded up | two images of scratch.  The state's first
 *   two int32 are (cycles done, done). */
#define KIMG_CLEAN_SCALES_MAX 6
#define KIMG_CLEAN_SCALES_MAX_RADIUS 64
#define KIMG_CLEAN_SCALES_PSF 1
#define KIMG_CLEAN_SCALES_RESIDUALS 2
int kimg_image_convolve_separable(const float *in, int64_t in_row_pitch, int64_t in_pol_pitch,
                                  float *out, int64_t out_row_pitch, int64_t out_pol_pitch,
                                  float *tmp, int64_t tmp_row_pitch, int64_t tmp_pol_pitch,
                                  int width, int height, int num_polarizations,
                                  const float *taps, int radius, void *stream);
size_t kimg_clean_scales_workspace_bytes(int width, int height, int num_polarizations,
                                         int patch_width, int patch_height, int border,
                                         int num_scales, const int *radii);
int kimg_clean_scales_setup(float *dirty, int64_t row_pitch, int64_t pol_pitch,
                            const float *psf, int64_t psf_row_pitch, int64_t psf_pol_pitch,
                            int width, int height, int num_polarizations,
                            int patch_width, int patch_height, int border,
                            int num_scales, const int *radii, const float *taps_host,
                            const float *cross_taps_host, int what,
                            const uint8_t *mask, int64_t mask_row_pitch,
                            void *workspace, size_t workspace_bytes, void *stream);
int kimg_clean_scales_cycles(float *dirty, float *model, int64_t row_pitch, int64_t pol_pitch,
                             int width, int height, int num_polarizations,
                             int patch_width, int patch_height, int border, int mode,
                             float loop_gain, float threshold, int num_scales, const int *radii,
                             const float *biases, int max_cycles,
                             const uint8_t *mask, int64_t mask_row_pitch,
                             void *workspace, size_t workspace_bytes, float *log,
                             int *cycles_done, void *stream);

/* ---- UV-plane continuum subtraction (contsub.hip): a low-order polynomial fitted across the
 * line-free channels of every baseline sample of a block of RAW visibilities, and subtracted from
 * all its channels, ahead of kimg_preprocess_convert (what CASA calls uvcontsub and MIRIAD uvlin).
 * The reference has none; the semantics are this library's, and katsdpimager_amd/continuum.py holds
 * them once more as numpy (uvcontsub_host).
 *
 * vis: complex64 [C][N][Q], weights: float32 [C][N][Q], C = num_channels, the loader's block layout.
 *   The inner [N][Q] plane is dense (plane_elements = N * Q); each array has its own channel pitch,
 *   the distance between channels in elements of the array (complex64 / float32), at least
 *   plane_elements (KIMG_EINVAL otherwise).  Elements of the padding are neither read nor written.
 *   Indices are 64-bit throughout: C * pitch may pass 2^31.
 * fit_mask_host: HOST uint8 [C], nonzero = a line-free channel that enters the fit.  It is read
 *   during the call and travels to the kernel by value, so a captured call keeps the mask it was
 *   captured with and the array may be freed on return.
 * basis: DEVICE float64 [K][C], K = order + 1, order 0 .. KIMG_UVCONTSUB_MAX_ORDER: the value of
 *   basis function k at channel c.  The host makes it (continuum.legendre_basis: Legendre
 *   polynomials of the channel index, or of the channel frequency, mapped linearly onto [-1, 1]).
 * For every element (n, q), all in float64:
 *   a channel is usable iff fit_mask[c] != 0, weights[c][n][q] > 0 and both parts of vis[c][n][q]
 *   are finite; m = the number of usable channels.  Over the usable channels in ascending c,
 *   A[k][l] = sum w B_k[c] B_l[c] (each term (w * B_k[c]) * B_l[c]) and b[k] = sum (w * B_k[c]) * v,
 *   b complex.  A a = b is solved by Cholesky without pivoting.
 *   m >= K: vis[c][n][q] = complex64((double) v - sum_k a[k] B_k[c]) for EVERY c, line channels
 *     included; the sum runs in ascending k from 0 and each part is rounded to float32 once.
 *     Non-finite visibilities outside the fit give whatever IEEE gives.  Weights are left alone.
 *   m < K: the element cannot be fitted.  Its vis stays as it is and weights[c][n][q] = 0 for every
 *     c, so that preprocessing drops it instead of imaging unsubtracted continuum.
 * counts: DEVICE uint64 [2]: the number of fitted and of flagged elements of the call are ADDED to
 *   it (one atomic add per wave and counter); the caller zeroes it.
 * Returns, before anything is enqueued: KIMG_EINVAL for order < 0, order > 3 or C < 1; then
 *   KIMG_EUNSUPPORTED when fewer than K entries of fit_mask_host are nonzero (nothing could ever be
 *   fitted) or C > KIMG_UVCONTSUB_MAX_CHANNELS; then KIMG_EINVAL for null pointers, a negative
 *   plane_elements or a pitch below it.  plane_elements = 0 is a successful call that does nothing.
 * Asynchronous on `stream`, no allocation, capturable.  The accumulation order is fixed: equal
 *   inputs give equal bits.  Traffic: 12 bytes per element and fit channel, 16 per element and
 *   channel. */
#define KIMG_UVCONTSUB_MAX_ORDER 3
#define KIMG_UVCONTSUB_MAX_CHANNELS 16384
int kimg_uvcontsub(void *vis, int64_t vis_channel_pitch, float *weights,
                   int64_t weights_channel_pitch, int num_channels, int64_t plane_elements,
                   const uint8_t *fit_mask_host, const double *basis, int order, uint64_t *counts,
                   void *stream);

/* ---- Phase-centre shift (phaseshift.hip): the RAW visibilities of a block re-phased to another
 * direction and the block's baseline coordinates rotated into that direction's frame, ahead of
 * kimg_uvcontsub and kimg_preprocess_convert (CASA phaseshift / fixvis, WSClean's chgcentre, MIRIAD
 * uvedit).  The reference has none; the semantics are this library's, and
 * katsdpimager_amd/phaseshift.py holds them once more as numpy (phase_shift_host).
 *
 * Frames.  For a direction (ra, dec) the frame M(ra, dec) has the rows
 *   e_u = (-sin ra, cos ra, 0), e_v = (-sin dec cos ra, -sin dec sin ra, cos dec),
 *   e_w = (cos dec cos ra, cos dec sin ra, sin dec).
 * Convention: a unit source at (l, m, n) of the frame gives exp(-2 pi i (l u + m v + (n - 1) w)),
 *   uvw in wavelengths.
 * Three directions: frame_centre, whose frame uvw_in (metres) is in; from_centre, the direction the
 *   visibilities are phased to now (usually frame_centre); new_centre, the direction they are to be
 *   phased to and whose frame uvw_out is in.  The host computes in float64
 *   rotation = M(new) . M(frame)^T (3 x 3) and
 *   delay[3] = lmn(new) - lmn(from), both directions' coordinates in the frame of frame_centre, each
 *   n - 1 taken as -(l^2 + m^2) / (1 + n) and the third entry as the difference of those.  With
 *   from == frame, delay = (l, m, n - 1) of the new centre and delay . uvw = w' - w.
 *
 * vis: complex64 [C][N][Q], C = num_channels, N = num_rows, Q = num_polarizations, updated in place.
 *   The inner [N][Q] plane is dense; vis_channel_pitch is the distance between channels in complex64
 *   elements, at least N * Q.  Elements of the padding are neither read nor written.  Indices are
 *   64-bit throughout.
 * uvw_in: DEVICE float32 [N][3], metres.  uvw_out: the same shape, or NULL: then only the
 *   visibilities are rotated.  uvw_out must not overlap uvw_in (the row of a sample is read by the
 *   threads of all its polarizations and written by one of them).
 * inv_wavelength: DEVICE float64 [C], 1 / wavelength of every channel in 1 / metres (f_c / c0).
 * params12_host: HOST float64 [12]: rotation row by row, then delay.  It is read during the call and
 *   travels to the kernel by value, so a captured call keeps its parameters and the array may be
 *   freed on return.
 * For every row n, with (u, v, w) = (double) uvw_in[n]:
 *   uvw_out[n][i] = (float) ((R[i][0] u + R[i][1] v) + R[i][2] w), one rounding per component;
 *   d = (delay[0] u + delay[1] v) + delay[2] w, in float64;
 * and for every channel c and polarization q
 *   vis[c][n][q] = vis[c][n][q] * exp(+2 pi i t), t = d * inv_wavelength[c].
 *   t is formed and reduced to [-0.5, 0.5] (t - rint(t)) in float64; only the reduced angle may go to
 *   float32.  Each component of the result lies within 10 * 2^-24 |vis[c][n][q]| of the float64
 *   value of this expression (DESIGN 5.15 derives it).
 * Weights are not this call's business: every sample is rotated, whatever its weight.  A non-finite
 *   coordinate makes the visibilities of its row and its rotated coordinates non-finite, a non-finite
 *   visibility component makes that visibility non-finite, and nothing else changes.
 * Returns KIMG_EINVAL, before any HIP call, for a null vis, uvw_in, inv_wavelength or params12_host,
 *   C < 1, Q < 1, N < 0, a pitch below N * Q, or uvw arrays that overlap.  N = 0 is a successful
 *   call that launches nothing.
 * Asynchronous on `stream`, no allocation, capturable; equal inputs give equal bits.  Traffic: 16
 *   bytes per element and channel, 12 per row read and 12 written. */
int kimg_phase_shift(void *vis, int64_t vis_channel_pitch, int num_channels, int64_t num_rows,
                     int num_polarizations, const float *uvw_in, float *uvw_out,
                     const double *inv_wavelength, const double *params12_host, void *stream);

/* ---- Primary-beam correction: frontend.py:587-608 + primary_beam.py (_sample_impl) of the reference,
 * whose host samples the beam with numba, uploads it and runs apply_primary_beam twice.  Here one
 * pass samples a radially symmetric beam model on the pixel grid and divides the model and the
 * residual image by its power.  katsdpimager_amd/primary_beam.py holds the contract once more as
 * numpy (sample_host, correct_host); the device agrees with it bit for bit (the NaN set included).
 *
 * row: DEVICE float32 [num_samples], the voltage pattern at radius i / inv_step (sine projection) at
 *   the channel's frequency; 2 <= num_samples <= KIMG_PRIMARY_BEAM_MAX_SAMPLES.  inv_step = the
 *   float32 nearest to 1 / step, formed by the caller, above 0.
 * Per pixel (x, y), in float32 with one rounding per operation (no fused multiply-add):
 *   l = (float) x * lm_scale + lm_bias,  m = (float) y * lm_scale + lm_bias   (kimg_layer_to_image's)
 *   s = sqrt(l * l + m * m) * inv_step
 *   s < num_samples - 1:  pos = (int) s, frac = s - pos,
 *                         v = row[pos] + (row[pos + 1] - row[pos]) * frac,  power = v * v
 *   otherwise (beyond the last sample, or s NaN):  power = NaN
 *   beam_power[y][x] = power                              (beam_power may be NULL: nothing stored)
 *   keep = power >= threshold                             (false for a NaN power)
 *   model[p][y][x] = keep ? model[p][y][x] / power : 0    for every polarization p
 *   dirty[p][y][x] = keep ? dirty[p][y][x] / power : NaN
 * A NaN beam blanks the model to 0 where kimg_apply_primary_beam on a NaN beam would leave NaN in
 * it (a NaN in the model spreads over the whole image in the restore step's transform); everywhere
 * else the pass equals sampling followed by kimg_apply_primary_beam on model (replacement 0) and
 * dirty (replacement NaN).
 * model and dirty: float32 [P][height][width] with the same row_pitch and pol_pitch (elements), both
 *   given or both NULL (NULL: sample only; beam_power is then required).  They and beam_power must
 *   not overlap.  Elements of the padding are neither read nor written.  Rows that start on 16-byte
 *   boundaries (pointers 16-byte aligned, pitches multiples of 4) move 16 bytes per lane; anything
 *   else is taken element by element, with the same results.
 * KIMG_EINVAL, before any HIP call: a null row; width or height below 1; num_polarizations outside
 *   1..4 (checked with or without images); num_samples outside 2..KIMG_PRIMARY_BEAM_MAX_SAMPLES;
 *   inv_step not above 0; one image without the other; neither images nor beam_power; a row pitch of
 *   a given array below the width; with P > 1, pol_pitch below (height - 1) * row_pitch + width.
 * Asynchronous on `stream`, no allocation, capturable; equal inputs give equal bits.  Traffic: 4
 *   bytes per pixel for the beam and 16 per pixel and polarization for the images. */
#define KIMG_PRIMARY_BEAM_MAX_SAMPLES 4096
int kimg_primary_beam(float *beam_power, int64_t beam_row_pitch,
                      float *model, float *dirty, int64_t row_pitch, int64_t pol_pitch,
                      int width, int height, int num_polarizations,
                      const float *row, int num_samples, float inv_step,
                      float lm_scale, float lm_bias, float threshold, void *stream);

/* ---- Spectral filter (spectral.hip): Hanning smoothing and channel averaging of a block of RAW
 * visibilities, ahead of kimg_uvcontsub and kimg_preprocess_convert and after kimg_phase_shift (CASA
 * hanningsmooth and mstransform(chanaverage=True) / split(width=n), MIRIAD hanning).  One operator: a
 * short non-negative FIR along the channel axis followed by a decimation, weighted and aware of
 * flags.  The reference has none; the semantics are this library's, and
 * katsdpimager_amd/spectral.py holds them once more as numpy (filter_host).
 *
 * Parameters (the Python side): taps, K float64 values, K odd, 1 <= K <= KIMG_SPECTRAL_MAX_TAPS,
 *   finite and >= 0, the centre tap h = K / 2 above 0; bin n, 1 <= n <= KIMG_SPECTRAL_MAX_BIN.  The
 *   host forms, in float64, the combined filter g = taps (*) ones(n), a full convolution of length
 *   L = K + n - 1 <= 72, and passes it as coeff_host with length = L, offset = h and step = n.
 * coeff_host: HOST float64 [length].  It is read during the call and travels to the kernel by value,
 *   so a captured call keeps its coefficients and the array may be freed on return.
 * vis_in: complex64 [C_in][N][Q], weights_in: float32 [C_in][N][Q], the loader's block layout; vis_out
 *   and weights_out: the same with C_out = num_channels_out channels, C_out * step <= C_in (the Python
 *   side takes C_out = C_in / n, rounded down; the trailing C_in % n channels enter only through the
 *   smoothing taps).  The inner [N][Q] plane is dense (plane_elements = N * Q); each of the four arrays
 *   has its own channel pitch in elements of the array, at least plane_elements.  Elements of the
 *   padding are neither read nor written, and the inputs are not written at all.  The operation is
 *   out of place: no output may start inside an input.  Indices are 64-bit throughout.
 * For every element (n, q) and output channel o, all in float64:
 *   input i of the window is channel c = o * step - offset + i, i = 0 .. length - 1.  It is usable
 *   iff 0 <= c < C_in, weights_in[c][n][q] > 0 and both parts of vis_in[c][n][q] are finite (the rule
 *   of kimg_uvcontsub).  Over the usable inputs in ascending i, with w and v the input's weight and
 *   visibility (w * v is exact in float64):
 *     cov = sum g_i,  S1 = sum (g_i * w),  S2 = sum g_i * (g_i * w),  N = sum g_i * (w * v)
 *   cov >= min_sum: the sample is kept,
 *     vis_out[o][n][q] = complex64(N / S1), each part rounded to float32 once (the device multiplies
 *     by 1 / S1, formed once: within 2^-52 of the quotient before that rounding);
 *     weights_out[o][n][q] = float32((S1 * S1) / S2), the inverse variance of the weighted mean of
 *     independent channels of variance 1 / w: sum w for plain averaging, w / 0.375 for Hanning on
 *     equal weights.
 *   otherwise it is flagged: vis_out = 0 and weights_out = 0 (preprocessing drops zero weights).
 *   min_sum: the host's min_coverage * (sum of all g_i), in float64; min_coverage in (0, 1].  The
 *   sums run in the stated order, so the kept set is the numpy statement's for any taps.
 * counts: DEVICE uint64 [2]: the number of kept and of flagged output samples of the call are ADDED
 *   to it (one atomic add per wave and counter); the caller zeroes it.
 * Returns, before any HIP call: KIMG_EINVAL for a null pointer; for length < 1, step < 1 or offset
 *   outside [0, length); then KIMG_EUNSUPPORTED for length > 72 or step > KIMG_SPECTRAL_MAX_BIN; then
 *   KIMG_EINVAL for a negative or non-finite coefficient, a min_sum that is not finite or not above
 *   0, num_channels_out < 1 or num_channels_out * step > num_channels_in, a negative plane_elements
 *   or a pitch below it; KIMG_EUNSUPPORTED for a plane beyond the grid limit (2^31 - 1 workgroups of
 *   256 elements) or more than 65535 * 64 output channels; KIMG_EINVAL for an output that starts
 *   inside an input.  plane_elements = 0 is then a successful call that does nothing.
 * Asynchronous on `stream`, no allocation, capturable; equal inputs give equal bits.  Traffic: 12
 *   bytes per element and input channel, 12 per element and output channel (Hanning and pure
 *   averaging read every input once; a smoothing filter with step > 1 re-reads the K - 1 channels
 *   neighbouring windows share, through the cache). */
#define KIMG_SPECTRAL_MAX_TAPS 9
#define KIMG_SPECTRAL_MAX_BIN 64
int kimg_spectral_filter(const void *vis_in, int64_t vis_in_channel_pitch, const float *weights_in,
                         int64_t weights_in_channel_pitch, int num_channels_in, void *vis_out,
                         int64_t vis_out_channel_pitch, float *weights_out,
                         int64_t weights_out_channel_pitch, int num_channels_out,
                         int64_t plane_elements, const double *coeff_host, int length, int offset,
                         int step, double min_sum, uint64_t *counts, void *stream);

/* ---- Statistical reweighting (statwt.hip): the weights of a block of RAW visibilities rescaled so
 * that they are inverse variances, from the scatter of the visibilities themselves across the
 * line-free channels (CASA statwt), after kimg_uvcontsub and ahead of kimg_preprocess_convert.  The
 * reference has none; the semantics are this library's, and katsdpimager_amd/statwt.py holds them once
 * more as numpy (statwt_host).  The device matches that twin bit for bit.
 *
 * vis: complex64 [C][N][P], read only.  weights: float32 [C][N][P], updated in place.  C =
 *   num_channels, N = num_rows, P = num_pols (1 .. 4), the loader's block layout.  The inner [N][P]
 *   plane is dense; each array has its own channel pitch in elements of the array, at least N * P.
 *   Elements of the padding are neither read nor written.  Indices are 64-bit throughout.
 * fit_mask_host: HOST uint8 [C], nonzero = a line-free channel that enters the statistic.  It is read
 *   during the call and travels to the kernels by value.
 * Groups.  A group is up to time_bin (1 .. KIMG_STATWT_MAX_BIN) consecutive rows of ONE baseline
 *   within the block; the statistic is taken per group and per polarization.  Loader blocks are
 *   stably sorted by baseline, so a baseline's samples are one contiguous, time-ordered run of rows,
 *   and the groups are that run cut every time_bin rows; the last group of a run may be shorter.
 *   Groups never span blocks: a baseline's rows in the next block start new groups.
 *   group_offsets: DEVICE int32 [G + 1], G = num_groups: group k is the rows g[k] .. g[k + 1] - 1,
 *     g[0] = 0, g[G] = N, strictly ascending, g[k + 1] - g[k] <= time_bin.
 *   row_group: DEVICE int32 [N]: the group of every row (g[row_group[r]] <= r < g[row_group[r] + 1]).
 *   The host makes both (statwt.group_offsets) and answers for them; the kernels clamp what they read
 *   from them to the arrays' bounds, so wrong tables give wrong weights and nothing else.
 * A sample (c, r, p) is usable iff fit_mask[c] != 0, its weight w is above 0 and finite, and both
 *   parts of its visibility v = (re, im) are finite.
 * Per group and polarization, all in float64, every product and every sum rounded on its own (no
 * fused multiply-add), in exactly this order:
 *   1. per row r, over its usable channels in ascending c, starting from 0:
 *        s0 += w,  sr += w * re,  si += w * im,  m += 1
 *   2. over the group's rows in ascending r, starting from 0: S0 = sum s0_r, SR, SI, M likewise;
 *        the mean is mu = (SR / S0, SI / S0)
 *   3. per row, over its usable channels in ascending c, starting from 0:
 *        dr = re - mu_r,  di = im - mu_i,  t = dr * dr,  t = t + di * di,  q += w * t
 *      then Q = sum q_r in ascending r
 *   4. chi2 = Q / (2.0 * (M - 1)): the weighted scatter per real component about the group's own
 *      mean.  For equal input weights w, w / chi2 is 1 / variance of the group's samples.
 *   5. the group is kept iff M >= min_samples (at least 2) and chi2_lo < chi2 < chi2_hi, both
 *      comparisons false for a NaN.  With the Python defaults (0, inf) constant data (chi2 == 0),
 *      S0 == 0 and overflow all flag the group; a narrower range is the caller's outlier cut.
 * For EVERY channel of the group's rows, line channels included:
 *   kept: weights[c][r][p] = float32((double) w / chi2) where w > 0; a weight that is not above 0
 *     (or is NaN) stays as it is, bit for bit.  Relative channel weights survive; only the absolute
 *     scale is measured.
 *   flagged: weights[c][r][p] = 0.
 * The visibilities are never written.
 * counts: DEVICE uint64 [2]: the number of kept and of flagged (group, polarization) pairs of the call
 *   are ADDED to it (one atomic add per wave and counter); the caller zeroes it.
 * chi2: DEVICE float64 [G][P], or NULL: chi2 of every pair, NaN where M < 2.
 * workspace: DEVICE, 8-byte aligned, at least KIMG_STATWT_WORKSPACE_PER_ELEMENT * N * P bytes
 *   (KIMG_EWORKSPACE otherwise): the per-row partial sums between the three launches.
 * Returns, before any HIP call: KIMG_EINVAL for a null vis, weights, fit_mask_host, group_offsets,
 *   row_group, workspace or counts; for C < 1, N < 0, P outside 1 .. 4, time_bin outside
 *   1 .. KIMG_STATWT_MAX_BIN, min_samples < 2 or a NaN in the chi2 range; KIMG_EUNSUPPORTED for
 *   N > 2^31 - 1 (rows are 32-bit in the tables); KIMG_EINVAL for a pitch below N * P;
 *   KIMG_EUNSUPPORTED for C > KIMG_UVCONTSUB_MAX_CHANNELS.  N = 0 is then a successful call that does
 *   nothing.  Then KIMG_EINVAL for G < 1, G > N or G * time_bin < N, KIMG_EWORKSPACE for a short
 *   workspace and KIMG_EINVAL for one that is not 8-byte aligned.
 * Asynchronous on `stream`, no allocation, capturable; equal inputs give equal bits.  Traffic: 12
 *   bytes per element and fit channel twice over, 8 per element and channel (4 for a flagged group).
 * Not done here: pooling polarizations, channel bins narrower than the band, groups across block
 *   boundaries, sliding windows, medians or other robust statistics. */
#define KIMG_STATWT_MAX_BIN 64
#define KIMG_STATWT_WORKSPACE_PER_ELEMENT 36
int kimg_statwt(const void *vis, int64_t vis_channel_pitch, float *weights,
                int64_t weights_channel_pitch, int num_channels, int64_t num_rows, int num_pols,
                const uint8_t *fit_mask_host, const int32_t *group_offsets, int64_t num_groups,
                const int32_t *row_group, int time_bin, int min_samples, double chi2_lo,
                double chi2_hi, double *chi2, void *workspace, size_t workspace_bytes,
                uint64_t *counts, void *stream);

/* ---- RFI flagging (rfiflag.hip): interference found in the time-frequency plane of every baseline of
 * a block of RAW visibilities by SumThreshold (AOFlagger; CASA flagdata tfcrop / rflag with
 * extendflags) and taken out by zeroing weights, after kimg_uvcontsub and ahead of kimg_statwt.  The
 * reference has none; the semantics are this library's, and katsdpimager_amd/rfiflag.py holds them
 * once more as numpy (rfiflag_host).  The device matches that twin bit for bit.
 *
 * vis, weights, the block layout, the pitches, group_offsets / row_group (statwt.group_offsets) and
 *   time_bin: as for kimg_statwt.  A group is one baseline's time-frequency plane of C channels by
 *   T <= time_bin rows, taken per polarization.  vis is never written.
 * mask_host: HOST uint8 [C], nonzero = a mask channel: searched for interference, part of the level.
 *   The other channels are PROTECTED (line channels: a bright line is constant in time and would be
 *   flagged): they never enter the level, no window flags them, inside a frequency window they count
 *   as flagged on entry, and only extension 1 below reaches them.
 * A sample (c, r, p) is usable iff its weight w is above 0 and finite and both parts of its
 *   visibility (re, im) are finite -- kimg_statwt's predicate.  An unusable sample keeps its weight
 *   bit for bit, is never flagged and never counted.
 * Statistic: z = w * (re * re + im * im) in float64, the sum and then the product rounded (the
 *   squares of float32 values are exact).
 * Level, per group and polarization, from the usable samples of mask channels: L0 = Z / M, Z the sum
 *   of z and M the number of samples; then for j = 1 .. level_iterations (0 ..
 *   KIMG_RFIFLAG_MAX_LEVEL_ITERATIONS) Lj = Z / M over those of them with z <= level_clip * L(j-1)
 *   (one product).  Sums in kimg_statwt's order: per row over channels in ascending c from 0, then
 *   over the group's rows in ascending r from 0; M an integer converted once.  If any of these M is
 *   0, or any L is not finite or not above 0, the (group, polarization) is SKIPPED: nothing of it is
 *   flagged by any step below.
 * SumThreshold: for m = 1, 2, 4, ... <= max_window (a power of two up to KIMG_RFIFLAG_MAX_WINDOW),
 *   k = log2 m, with chi = factors_host[k] * L and the limit (double) m * chi.  factors_host: HOST
 *   float64 [log2(max_window) + 1], each above 0 (threshold / rho^k, made by the caller), read
 *   during the call.  Passes run in ascending m; each reads the flags that entered it and ORs its
 *   own in afterwards, so within a pass nothing depends on the order of evaluation.  In a pass, for
 *   each direction of `directions` (KIMG_RFIFLAG_TIME | KIMG_RFIFLAG_FREQ):
 *     frequency: for every row and every s with s + m <= C, the sum over c = s .. s + m - 1 in
 *       ascending order from 0.0, to which a usable sample of a mask channel that is not flagged on
 *       entry adds z - L (one subtraction, rounded) and every other sample adds chi.  If at least
 *       one sample added its own term and the sum is above the limit, every usable sample of a mask
 *       channel in the window is flagged.  (z of noise is exponentially distributed, mean and
 *       scatter both L: z - L has mean 0 and chi counts in sigma, as SumThreshold's factors do.)
 *     time: the same over the rows t = s .. s + m - 1 of one group, s + m <= the group's end, in one
 *       mask channel.
 * Extension, after the last pass, each step on the flags as the previous one left them:
 *   1. extend_freq in (0, 1], or 0 for none: a (row, polarization) with F of its U usable samples of
 *      mask channels flagged and (double) F > extend_freq * (double) U has ALL its usable samples
 *      flagged, protected channels included.
 *   2. extend_time, likewise: a (group, mask channel, polarization) with F of its U usable rows
 *      flagged and (double) F > extend_time * (double) U has all its usable rows flagged.
 *   3. extend_pols != 0: a sample flagged in any polarization is flagged in every polarization in
 *      which it is usable and whose (group, polarization) is not skipped.
 * Outputs.  weights: +0.0f where flagged, else untouched.  flags: DEVICE uint8 [C][N][P], dense:
 *   1 = flagged by this call, else 0.  level: DEVICE float64 [G][P], the final L, NaN where skipped.
 *   counts: DEVICE uint64 [3]: usable samples kept, usable samples flagged (all channels) and skipped
 *   (group, polarization) pairs of the call are ADDED to it (one atomic add per wave and counter).
 * workspace: DEVICE, 8-byte aligned, at least KIMG_RFIFLAG_WORKSPACE_PER_ELEMENT * C * N * P +
 *   KIMG_RFIFLAG_WORKSPACE_PER_ROW * N * P bytes (KIMG_EWORKSPACE otherwise): z and a byte of flag
 *   state per sample, two sets of the level's per-row partial sums.
 * Returns, before any HIP call: KIMG_EINVAL for a null pointer argument; for C < 1, N < 0, P outside
 *   1 .. 4, time_bin outside 1 .. KIMG_STATWT_MAX_BIN, max_window not a power of two in 1 ..
 *   KIMG_RFIFLAG_MAX_WINDOW, directions outside 1 .. 3, level_iterations outside its range, a
 *   level_clip or a factor not above 0 (or NaN), an extension share outside [0, 1];
 *   KIMG_EUNSUPPORTED for N > 2^31 - 1; KIMG_EINVAL for a pitch below N * P; KIMG_EUNSUPPORTED for
 *   C > KIMG_UVCONTSUB_MAX_CHANNELS.  N = 0 is then a successful call that does nothing.  Then
 *   KIMG_EINVAL for G < 1, G > N or G * time_bin < N, KIMG_EWORKSPACE for a short workspace and
 *   KIMG_EINVAL for one that is not 8-byte aligned.
 * Asynchronous on `stream`, plain launches, no allocation; equal inputs give equal bits.
 * Not done here: a surface-fit high-pass, medians, groups across block boundaries, a refit of the
 *   continuum on the flagged residuals. */
#define KIMG_RFIFLAG_MAX_WINDOW 32
#define KIMG_RFIFLAG_MAX_LEVEL_ITERATIONS 4
#define KIMG_RFIFLAG_WORKSPACE_PER_ELEMENT 9
#define KIMG_RFIFLAG_WORKSPACE_PER_ROW 24
#define KIMG_RFIFLAG_TIME 1
#define KIMG_RFIFLAG_FREQ 2
int kimg_rfi_flag(const void *vis, int64_t vis_channel_pitch, float *weights,
                  int64_t weights_channel_pitch, int num_channels, int64_t num_rows, int num_pols,
                  const uint8_t *mask_host, const int32_t *group_offsets, int64_t num_groups,
                  const int32_t *row_group, int time_bin, const double *factors_host, int max_window,
                  int directions, int level_iterations, double level_clip, double extend_freq,
                  double extend_time, int extend_pols, uint8_t *flags, double *level,
                  void *workspace, size_t workspace_bytes, uint64_t *counts, void *stream);

/* ---- Moment maps (moments.hip): a spectral cube of images reduced along its channel axis to the
 * maps a spectral-line user reads (CASA immoments, MIRIAD moment): integrated intensity (moment 0),
 * intensity-weighted coordinate (1), dispersion (2), peak (8) and coordinate of the peak (9), each
 * taken over the samples above a per-channel cut.  The reference has none; the semantics are this
 * library's, and katsdpimager_amd/cube.py holds them once more as numpy (moments_host).
 *
 * cube: DEVICE float32 [C][M], read only, never written: C = num_channels (1 ..
 *   KIMG_MOMENTS_MAX_CHANNELS) planes of M = plane_elements values (for images [P][H][W], dense,
 *   M = P * H * W), channel_pitch elements apart, channel_pitch >= M.  Elements of the padding are
 *   neither read nor written.  Indices are 64-bit throughout.
 * Tables, per channel: x DEVICE float64 [C], the coordinate of every channel (km/s or Hz: the
 *   library does not care); cut DEVICE float32 [C], made by the caller -- float32(clip_sigma) *
 *   noise[c] as one float32 product, an absolute cut, or -inf for none; filled_host HOST uint8 [C],
 *   nonzero = the plane holds an image.  filled_host is read during the call and travels to the
 *   kernel by value, a bit per channel; x and cut are read by the kernel (scalar loads).
 * Per element m of the plane on its own, over the channels c = first .. stop - 1 (0 <= first < stop
 *   <= C) in ascending order, with I = cube[c][m]:
 *   I is usable iff filled[c] and I is finite.
 *   Selection value: s = (double) I, or with select_hanning != 0
 *       s = ((0.25 * a) + (0.5 * I)) + (0.25 * b)    in float64, every product and sum rounded,
 *     a = cube[c - 1][m] and b = cube[c + 1][m], each replaced by I itself where that channel is
 *     outside first .. stop - 1, not filled, or not finite at m (the replicate rule).
 *   The sample ENTERS iff I is usable and s > (double) cut[c] (false for a NaN cut).
 *   For each sample that enters, in float64, nothing fused:
 *       n += 1;  d = x[c] - x_ref;  S0 += I;  t = I * d;  S1 += t;  S2 += t * d
 *     and the peak (float32, starting below everything) is replaced, with its channel, only if
 *     I > peak: the first channel wins a tie.
 *   x_ref = x[(first + stop) / 2] (integer division).  width: the caller's, float64: the absolute
 *     mean spacing |x[stop - 1] - x[first]| / (stop - first - 1) of the range, or the channel width
 *     on that axis for a range of one channel.
 * Outputs, float32 [M] each, every value ONE rounding of a float64:
 *     moment 0   S0 * width
 *     moment 1   x_ref + r,  r = S1 / S0
 *     moment 2   sqrt(v),  v = S2 / S0 - r * r (division, product, difference), 0 in place of v < 0
 *     moment 8   the peak
 *     moment 9   x of the peak's channel
 *   and count, int32 [M] = n.  Every moment is NaN where n == 0; moments 1 and 2 are NaN unless
 *   S0 > 0.  outputs: the KIMG_MOMENT_* bits of what is written; the pointer of a bit that is not set
 *   is ignored (NULL will do) and nothing is written through it.
 * Agreement with the twin: bit for bit for moments 0, 1, 8, 9 and count (IEEE additions, products
 *   and divisions in one fixed order).  Moment 2 too: the float64 sqrt of this build is the
 *   compiler's expansion of llvm.sqrt.f64 (read in the assembly of moments.hip) -- y = v_rsq_f64(x),
 *   g = x y, h = y / 2, one Goldschmidt step on both in FMAs, then twice the residual correction
 *   d = fma(-g, g, x), g = fma(d, h, g), the input scaled by 2^256 below 2^-767 -- whose last FMA
 *   rounds an estimate already inside an ulp once more against the exact residual: correctly
 *   rounded, as numpy's sqrt is.  The tests assert equal bits, not a bound.
 * Kernel forms (the host picks): four consecutive elements per thread with 16-byte loads and stores
 *   when cube, channel_pitch * 4 and every requested output are 16-byte aligned, for the first
 *   4 * (M / 4) elements; one element per thread for the tail and for everything else.  One launch
 *   per form, every voxel of the range read once (never for a channel that is not filled), no LDS,
 *   no atomics, no workspace.
 * Returns, before any HIP call: KIMG_EINVAL for a null cube, x, cut or filled_host; for C < 1,
 *   M < 0, a range outside 0 <= first < stop <= C, a pitch below M, a width that is NaN, outputs
 *   without any KIMG_MOMENT_* bit or with others, or a requested output that is NULL (or not
 *   4-byte aligned); KIMG_EUNSUPPORTED for C > KIMG_MOMENTS_MAX_CHANNELS or M beyond the grid limit
 *   (2^31 - 1 workgroups of 256 elements).  M = 0 is then a successful call that does nothing.
 * Asynchronous on `stream`, no allocation, capturable; equal inputs give equal bits.
 * Not done here (a common restoring beam across planes is kimg_cube_smooth's; a selection smoothed
 *   in space and along the spectrum is the detection mask's, "Detection mask" below, which reaches
 *   this call through kimg_cube_mask_apply): position-velocity cuts, cubes across several GPUs.  The
 *   median, minimum and robust
 *   sigma along the spectrum (CASA moments 3 and 10) are kimg_spectrum_stats'; still missing are
 *   moments 4 to 7, the coordinate of the minimum (11) and a per-pixel cut made from those maps. */
#define KIMG_MOMENTS_MAX_CHANNELS 4096
#define KIMG_MOMENT_0 1
#define KIMG_MOMENT_1 2
#define KIMG_MOMENT_2 4
#define KIMG_MOMENT_8 8
#define KIMG_MOMENT_9 16
#define KIMG_MOMENT_COUNT 32
int kimg_moments(const float *cube, int64_t channel_pitch, int num_channels, int64_t plane_elements,
                 int first, int stop, const double *x, const float *cut, const uint8_t *filled_host,
                 double width, int select_hanning, int outputs, float *moment0, float *moment1,
                 float *moment2, float *moment8, float *moment9, int32_t *count, void *stream);

/* ---- Image-plane continuum subtraction (imcontsub.hip): per element of the plane of a spectral
 * cube, a low-order polynomial fitted across the line-free channels and subtracted from every filled
 * channel (CASA imcontsub, MIRIAD contsub) -- the image-plane partner of kimg_uvcontsub, for a cube
 * that already exists and for continuum anywhere in the field.  The reference has none; the semantics
 * are this library's, and katsdpimager_amd/imcontsub.py holds them once more as numpy
 * (imcontsub_host).
 *
 * cube: DEVICE float32 [C][M]: C = num_channels (1 .. KIMG_MOMENTS_MAX_CHANNELS) planes of
 *   M = plane_elements values (for images [P][H][W], dense, M = P * H * W), channel_pitch elements
 *   apart, channel_pitch >= M.  line: DEVICE float32 [C][M] with a pitch of its own, the result:
 *   either exactly `cube` (the same pointer AND the same pitch: in place) or a buffer that shares no
 *   byte with the cube's C planes (any other overlap is KIMG_EINVAL).  Elements of the padding are
 *   neither read nor written.  Indices are 64-bit throughout.
 * Tables, per channel: filled_host HOST uint8 [C], nonzero = the plane holds an image; fit_host HOST
 *   uint8 [C], nonzero = a line-free channel; w DEVICE float64 [C], the weight of every channel, and
 *   w_host HOST float64 [C], the same numbers where the call itself can read them; basis DEVICE
 *   float64 [K][C], K = order + 1, order 0 .. KIMG_IMCONTSUB_MAX_ORDER: the value of basis function
 *   k at channel c (continuum.legendre_basis, by channel index or by frequency).  bref0 .. bref3: the
 *   basis functions 0 .. K - 1 at the reference position, by value (the rest is ignored).
 *   A channel ENTERS THE FIT iff fit_host[c], filled_host[c] and 0 < w_host[c] < inf.  The call folds
 *   the three into one bit mask; it and the filled mask travel to the kernel by value, so the host
 *   tables may be freed on return and a captured call keeps the masks it was captured with.  w and
 *   basis are read by the kernel (scalar loads).
 * Per element m of the plane on its own, all in float64, nothing fused.  I = cube[c][m] is usable
 *   iff it is finite.  Over the channels that enter the fit, in ascending c, for every usable I:
 *       n += 1;  wb = w[c] * B[k][c];  A[k][l] += wb * B[l][c] (l <= k);  b[k] += wb * I
 *   -- the steps of kimg_uvcontsub with one real right-hand side.  The element is FITTED iff
 *   n >= max(K, min_samples), 1 <= min_samples <= C.  Then A a = b is solved by Cholesky without
 *   pivoting and two triangular solves, as in kimg_uvcontsub.
 * Outputs for a fitted element: for every filled channel c of the whole band with finite I,
 *       line[c][m] = float32(I - model_c),  model_c = sum_k a[k] * B[k][c]
 *   summed from 0 in ascending k; an I that is not finite is stored as it is, bit for bit.  A channel
 *   that is not filled is neither read nor written.
 *       continuum[m]       = float32(sum_k a[k] * bref[k])     (from 0, ascending k)
 *       coefficients[k][m] = float32(a[k]),  planes coefficient_pitch elements apart (>= M)
 *       count[m]           = n  (int32)
 *       rms[m]             = float32(sqrt(R / (n - K))),  R = the sum of r * r, r = I - model_c, over the
 *                            usable samples of the channels that enter the fit, in ascending c;
 *                            NaN unless n > K.
 *   For an element that is NOT fitted: every filled channel of line at m becomes the quiet NaN
 *   0x7fc00000; continuum, coefficients and rms become NaN; count is still n.
 *   outputs: the KIMG_IMCONTSUB_* bits of the maps that are written, at least one; the pointer of a
 *   bit that is not set is ignored (NULL will do) and nothing is written through it.
 * Kernel forms (the host picks): four consecutive elements per thread with 16-byte loads and stores
 *   when cube, line, both pitches * 4, every requested map and, with coefficients,
 *   coefficient_pitch * 4 are 16-byte aligned, for the first 4 * (M / 4) elements; one element per
 *   thread for the tail and for everything else.  One launch per form; a voxel of a fit channel is
 *   read twice, of any other filled channel once, and written once.  No LDS, no atomics, no workspace.
 * Returns, before any HIP call: KIMG_EINVAL for order < 0, order > 3, C < 1 or a null host table;
 *   then KIMG_EUNSUPPORTED for C > KIMG_MOMENTS_MAX_CHANNELS, for fewer than K channels that enter the
 *   fit (nothing could ever be fitted) or for M beyond the grid limit (2^31 - 1 workgroups of 256
 *   elements); then KIMG_EINVAL for a null cube, line, w or basis, M < 0, min_samples outside 1 .. C,
 *   a pitch below M, outputs without any KIMG_IMCONTSUB_* bit or with others, a pointer that is not
 *   aligned to its element, a requested map that is NULL, or a line that overlaps the cube without
 *   being the cube.  M = 0 is then a successful call that does nothing.
 * Asynchronous on `stream`, no allocation, capturable.  The order of every sum is fixed: equal inputs
 *   give equal bits.  Agreement with the twin: the bound of kimg_uvcontsub's tests,
 *   |dev - t| <= 2^-24 |t| + 1e-9 S against the twin's value before its one rounding.
 * Not done here: robust polynomial fits and iterative clipping (the order-0 robust case, the
 *   per-pixel median across the band, is kimg_spectrum_stats' line), per-pixel weights, a fit across
 *   several cubes. */
#define KIMG_IMCONTSUB_MAX_ORDER 3
#define KIMG_IMCONTSUB_CONTINUUM 1
#define KIMG_IMCONTSUB_COEFFICIENTS 2
#define KIMG_IMCONTSUB_RMS 4
#define KIMG_IMCONTSUB_COUNT 8
int kimg_imcontsub(const float *cube, int64_t channel_pitch, float *line, int64_t line_channel_pitch,
                   int num_channels, int64_t plane_elements, const uint8_t *filled_host,
                   const uint8_t *fit_host, const double *w_host, const double *w,
                   const double *basis, int order, double bref0, double bref1, double bref2,
                   double bref3, int min_samples, int outputs, float *continuum, float *coefficients,
                   int64_t coefficient_pitch, float *rms, int32_t *count, void *stream);

/* ---- Cube smoothing to a common beam (cube_smooth.hip): every filled plane of a spectral cube
 * convolved with a small kernel of its own, so that all planes end with one restoring beam (CASA
 * imsmooth(targetres=True) / commonbeam, MIRIAD convol options=final) -- the step between imaging
 * and the cube operators above, which assume that a pixel means the same in every channel.  The
 * kernel that takes the beam of channel c to the common beam T is the Gaussian of covariance
 * Sigma_T - Sigma_c: a fraction of a pixel to a few pixels over a spectral-line band, so the
 * convolution is direct, in the image domain, not kimg_convolve_beam's.  The reference has none; the
 * semantics are this library's, and katsdpimager_amd/smooth.py holds them once more as numpy
 * (cube_smooth_host), with the host code that chooses the common beam (common_beam) and makes the
 * taps (kernel_tables).
 *
 * cube: DEVICE float32 [C][P][H][W], read only: C = num_channels (1 .. KIMG_MOMENTS_MAX_CHANNELS)
 *   channels channel_pitch elements apart, channel_pitch >= P * H * W; inside a channel the
 *   P = num_polarizations planes of H = height rows of W = width pixels are dense, as in
 *   kimg_moments.  out: DEVICE float32 of the same shape with a pitch of its own, which shares no
 *   byte with the cube's C channels (in-place operation is not done; any overlap is KIMG_EINVAL).
 *   Elements of the padding are neither read nor written.  Indices are 64-bit throughout.
 * Tables, per channel: filled_host HOST uint8 [C], nonzero = the plane holds an image; radius_host
 *   HOST int32 [C], R_c = 0 .. KIMG_CUBE_SMOOTH_MAX_RADIUS (read for filled channels only); both
 *   travel to the kernel by value, 5 bits a channel, so they may be freed on return and a captured
 *   call keeps the ones it was captured with.  taps DEVICE float32 [C][taps_pitch]: channel c uses
 *   its first (2 R_c + 1)^2 entries, row-major, taps[c][(dy + R)(2R + 1) + (dx + R)], and
 *   taps_pitch must hold them.  They are read by the kernel (scalar loads).
 * Per filled channel c, polarization p and pixel (y, x), R = R_c, every operation in float32,
 *   every product and every sum rounded, nothing fused, dy ascending and within it dx ascending:
 *       acc = +0.0f
 *       acc = acc + (taps[c][(dy + R)(2R + 1) + (dx + R)] * I[c][p][y + dy][x + dx])
 *   where a sample outside the plane is +0.0f, multiplied and added like any other (so an infinite
 *   tap over the border makes a NaN).  The accumulator starts as +0.0 and +0.0 + -0.0 = +0.0, so it
 *   is never -0.0: a sample of -0.0 comes out as +0.0, in a scaled copy (R = 0) too.
 *   Samples that are not finite take part as they are: a NaN spreads over its footprint.  A result
 *   that is NaN is stored as 0x7fc00000, everything else as computed.  R = 0 is the same formula
 *   with one tap: a scaled copy.  A channel that is not filled is neither read nor written.
 * Agreement with the twin: bit for bit (IEEE products and sums in one fixed order).
 * Kernel forms (the host picks): 16-byte loads and stores when cube, out, both pitches * 4 and
 *   W * 4 are 16-byte aligned, one pixel per load and store for everything else.  One launch for all
 *   channels and polarizations; a workgroup stages a tile of 64 x 64 outputs with its halo in LDS
 *   (36880 bytes); no atomics, no workspace.
 * Returns, before any HIP call: KIMG_EINVAL for a null cube, out, filled_host, radius_host or taps,
 *   C, P, H or W below 1, C > KIMG_MOMENTS_MAX_CHANNELS, a pointer that is not 4-byte aligned, a
 *   pitch below P * H * W or so long that the cube's extent in bytes leaves int64, a filled channel whose radius is outside 0 .. 16 or whose taps do not
 *   fit taps_pitch, or an out that overlaps the cube; then KIMG_EUNSUPPORTED for P > 65535 or more
 *   than 2^31 - 1 tiles a plane.  No filled channel is then a successful call that does nothing.
 * Asynchronous on `stream`, no allocation, capturable; equal inputs give equal bits.
 * Not done here: minimum-area common beams of differently shaped ellipses (smooth.common_beam
 *   scales the largest beam), kernels beyond R = 16 (kimg_convolve_beam's work), sub-pixel kernels
 *   sampled better than at pixel centres, the noise of the smoothed planes, in-place operation,
 *   cubes across several GPUs. */
#define KIMG_CUBE_SMOOTH_MAX_RADIUS 16
int kimg_cube_smooth(const float *cube, int64_t channel_pitch, float *out, int64_t out_channel_pitch,
                     int num_channels, int num_polarizations, int height, int width,
                     const uint8_t *filled_host, const int32_t *radius_host, const float *taps,
                     int64_t taps_pitch, void *stream);

/* ---- Cube plane statistics (cube_stats.hip): for every plane of a spectral cube a robust noise and
 * its companion statistics, in one call (CASA imstat per channel, MIRIAD imstat / sigest) -- what
 * measures the noise that kimg_moments' clip_sigma cut and kimg_imcontsub's noise weights read, on a
 * cube that did not come plane by plane from the imager: a smoothed cube, a continuum-subtracted one,
 * one filled from the host.  The reference has none; the semantics are this library's, and
 * katsdpimager_amd/cube_stats.py holds them once more as numpy (cube_stats_host).
 *
 * cube: DEVICE float32 [C][P][H][W], read only, never written: C = num_channels
 *   (1 .. KIMG_MOMENTS_MAX_CHANNELS) channels channel_pitch elements apart, channel_pitch >= P * H * W;
 *   inside a channel the P planes of H rows of W pixels are dense, as in kimg_moments.  Elements of
 *   the padding are not read.  filled_host: HOST uint8 [C], nonzero = the plane holds an image; it
 *   travels by value.  Channels first .. stop - 1 are measured.
 * Groups: G = 1 a channel with pool_polarizations (all P planes together: one number a channel, as
 *   the imager's own estimate), else G = P.  A group's candidates are the pixels (y, x) of its
 *   plane(s) with border <= y < H - border, border <= x < W - border (border in pixels, >= 0,
 *   2 * border < min(H, W)) and, with a region (DEVICE uint8 [H][W], dense, shared by all planes; null
 *   for none), region[y][x] != 0.
 * Samples: the candidates whose value is finite; NaN of any sign and payload, +Inf and -Inf are left
 *   out.  n is their number.
 * Order: by key(x) = bits ^ (bits >> 31 ? 0xffffffff : 0x80000000), the monotone map of the float32
 *   bit pattern: -0 lies below +0.  The median of a multiset v of n >= 1 float32 values is
 *   (lo + hi) / 2 in float32 with lo = v[(n - 1) / 2] and hi = v[n / 2] in that order (kimg_noise_est's
 *   rule, np.median of float32 data).
 * Outputs, DEVICE [C][G] each, group c * G + g: count (uint32) = n; min and max, the samples of
 *   smallest and largest key; median, the median of the samples; sigma, by estimator:
 *     KIMG_CUBE_STATS_MEDIAN_ABS  median(|x|) * KIMG_CUBE_STATS_TO_RMS, one float32 product, |x| the
 *                                 value with its sign bit cleared (the imager's kimg_noise_est);
 *     KIMG_CUBE_STATS_MAD         median(|x - m|) * KIMG_CUBE_STATS_TO_RMS, m the group's median,
 *                                 x - m one float32 subtraction, its sign bit cleared (it may be +Inf,
 *                                 which is then a value like any other).
 *   A group with n = 0, and every group of a channel that is not filled or outside the range, gets NaN
 *   (0x7fc00000) in the four float outputs and count 0; a channel that is not filled is not read.
 * Exactness: everything is selection; nothing is summed and nothing rounds but the operations named
 *   above.  The results depend neither on the launch geometry nor on the kernel form, and the twin
 *   gives the same bits, always.  On a plane without non-finite values, pooled, without a region and
 *   with the same border in pixels, sigma under MEDIAN_ABS is kimg_noise_est's, bit for bit.
 * Kernel: a batched byte-wise radix select over all groups, two launches a pass whatever C is;
 *   MEDIAN_ABS reads the cube 4 times (both selects share every load), MAD 8 times.  16-byte loads
 *   when cube, channel_pitch * 4 and W * 4 are 16-byte aligned, one element a load otherwise.
 * scratch: DEVICE, kimg_cube_stats_scratch_bytes(C, G) bytes (0 for arguments out of range), 8-byte
 *   aligned; the call initialises it.
 * Returns, before any HIP call: KIMG_EINVAL for a null pointer (region excepted), C, P, H or W below
 *   1, C > KIMG_MOMENTS_MAX_CHANNELS, a range that is empty or leaves the band, an unknown estimator,
 *   a border below 0 or with 2 * border >= min(H, W), a misaligned pointer, a pitch below P * H * W or
 *   so long that the cube's extent in bytes leaves int64; then KIMG_EUNSUPPORTED for a group of 2^32
 *   elements or more (so for every group of 2^32 candidates or more) and for G > 65535.
 * Asynchronous on `stream`, no allocation, capturable; the caller reads the 5 * C * G numbers.
 * Not done here: iterative sigma clipping; means and rms (an ordered float64 reduction, another
 *   contract); the noise of a smoothed plane derived rather than measured; cubes across several
 *   GPUs.  Statistics along the channel axis per pixel are kimg_spectrum_stats'. */
#define KIMG_CUBE_STATS_MEDIAN_ABS 0
#define KIMG_CUBE_STATS_MAD 1
#define KIMG_CUBE_STATS_TO_RMS 1.4826022185056031f
size_t kimg_cube_stats_scratch_bytes(int num_channels, int groups_per_channel);
int kimg_cube_stats(const float *cube, int64_t channel_pitch, int num_channels, int num_polarizations,
                    int height, int width, const uint8_t *filled_host, int first, int stop,
                    int pool_polarizations, int estimator, int border, const uint8_t *region,
                    void *scratch, uint32_t *count, float *min, float *max, float *median,
                    float *sigma, void *stream);

/* ---- Spectrum statistics (spectrum_stats.hip): for every element of the plane of a spectral cube the
 * statistics of its own spectrum -- count, min, max, median and a robust sigma along the channel axis
 * -- as maps [P][H][W], and optionally the cube with the median subtracted from every filled channel:
 * the per-pixel noise map that source finders scale by, and the continuum estimate that needs no line
 * ranges (CASA immoments' moment 3, MIRIAD contsub's median mode).  kimg_cube_stats selects along a
 * plane, one number a plane; this selects along a column, one number an element.  The reference has
 * none; the semantics are this library's, and katsdpimager_amd/spectrum_stats.py holds them once more
 * as numpy (spectrum_stats_host).
 *
 * cube: DEVICE float32 [C][M]: C = num_channels (1 .. KIMG_MOMENTS_MAX_CHANNELS) planes of
 *   M = plane_elements values, channel_pitch elements apart, channel_pitch >= M, as in kimg_moments.
 *   Elements of the padding are neither read nor written.  Indices are 64-bit throughout.  The cube
 *   is never written, unless `line` is the cube (below).
 * Tables, per channel: stat_host and filled_host, HOST uint8 [C], read during the call; they travel
 *   to the kernels by value, a bit per channel.  A channel ENTERS the statistics iff
 *   first <= c < stop (0 <= first < stop <= C), stat_host[c] and filled_host[c].  S is the number of
 *   entering channels; S = 0 is legal and gives n = 0 everywhere.
 * Per element m on its own.  The samples are the finite cube[c][m] of the entering channels (NaN of
 *   any sign or payload, +Inf and -Inf are left out), n their count.  Order is by kimg_cube_stats'
 *   key, key(x) = bits ^ (bits >> 31 ? 0xffffffff : 0x80000000): -0 lies below +0.  With v the samples
 *   in that order:
 *     median  (v[(n - 1) / 2] + v[n / 2]) / 2 in float32 (kimg_cube_stats' rule; it may overflow to Inf)
 *     min, max  the samples of smallest and largest key
 *     sigma   KIMG_CUBE_STATS_MAD: median(|x - median|) * KIMG_CUBE_STATS_TO_RMS, x - median one
 *             float32 subtraction with its sign bit cleared (+Inf is a value like any other; it is
 *             never NaN); KIMG_CUBE_STATS_MEDIAN_ABS: median(|x|) times the same constant.  The
 *             absolute values are ordered by 0x80000000 | abs bits and their median follows the rule
 *             above; the product is one float32 product.
 *     count   n (int32), always.
 *   min_samples (>= 1): the four float maps hold 0x7fc00000 where n < min_samples.
 * outputs: the KIMG_SPECTRUM_* bits of the maps [M] that are written, at least one.  The pointer of a
 *   bit that is not set is ignored (NULL will do) and nothing is written through it; without
 *   KIMG_SPECTRUM_SIGMA the sigma select is not run.
 * line: NULL, or DEVICE float32 [C][M] with a pitch of its own: either exactly `cube` (the same
 *   pointer AND the same pitch: in place) or a buffer that shares no byte with the cube's C planes.
 *   For every filled channel c of 0 .. C - 1 -- not only the entering ones, not only the range --
 *   line[c][m] = cube[c][m] - median[m], one float32 subtraction, where n >= min_samples, and
 *   0x7fc00000 where not.  Channels that are not filled are neither read nor written.  The
 *   subtraction reads the median map: a line needs KIMG_SPECTRUM_MEDIAN among the outputs.
 * form: KIMG_SPECTRUM_FORM_RESIDENT keeps the keys of a wave's elements in LDS and reads the cube once
 *   (S up to kimg_spectrum_stats_resident_limit()); KIMG_SPECTRUM_FORM_STREAMING is a radix select on
 *   4-bit digits that re-reads the entering channels 9 times for the median and 9 more for sigma, for
 *   any S; KIMG_SPECTRUM_FORM_AUTO takes the resident form for S <= 63 and the streaming form above,
 *   where the two were measured level.  Load forms as in
 *   kimg_moments: four elements per thread with 16-byte accesses when cube, line, their pitches * 4
 *   and every requested map are 16-byte aligned, for the first 4 * (M / 4) elements; one element per
 *   thread for the tail and for everything else.
 * Agreement: everything is exact selection plus the single float32 operations named above.  Device
 *   and twin have equal bits always, in every form, layout and launch geometry, and the two forms
 *   have each other's bits.  (The NaN of a non-finite cube value minus the median is a NaN; its
 *   payload is the hardware's.)
 * Returns, before any HIP call: KIMG_EINVAL for a null cube, stat_host or filled_host; C < 1, M < 0; a
 *   range outside 0 <= first < stop <= C; a pitch below M; an unknown estimator; min_samples < 1;
 *   outputs without any KIMG_SPECTRUM_* bit or with others; an unknown form; a requested map that is
 *   NULL; a pointer that is not 4-byte aligned; a line without KIMG_SPECTRUM_MEDIAN, with a pitch
 *   below M, or one that overlaps the cube without being the cube; then KIMG_EUNSUPPORTED for
 *   C > KIMG_MOMENTS_MAX_CHANNELS, for M beyond the grid limit (2^31 - 1 workgroups of 64 elements)
 *   and for KIMG_SPECTRUM_FORM_RESIDENT with S above the limit.  M = 0 is then a successful call
 *   that does nothing.
 * Asynchronous on `stream`, no allocation, no workspace, capturable; equal inputs give equal bits.
 * Not done here: moments 4 to 7 (absolute mean deviations and the like), the coordinate of the
 *   minimum (moment 11), a per-pixel cut in kimg_moments made from these maps, iterative clipping,
 *   robust polynomial fits. */
#define KIMG_SPECTRUM_MEDIAN 1
#define KIMG_SPECTRUM_SIGMA 2
#define KIMG_SPECTRUM_MIN 4
#define KIMG_SPECTRUM_MAX 8
#define KIMG_SPECTRUM_COUNT 16
#define KIMG_SPECTRUM_FORM_AUTO 0
#define KIMG_SPECTRUM_FORM_RESIDENT 1
#define KIMG_SPECTRUM_FORM_STREAMING 2
int kimg_spectrum_stats_resident_limit(void);
int kimg_spectrum_stats(const float *cube, int64_t channel_pitch, int num_channels,
                        int64_t plane_elements, int first, int stop, const uint8_t *stat_host,
                        const uint8_t *filled_host, int estimator, int min_samples, int outputs,
                        float *median, float *sigma, float *min, float *max, int32_t *count,
                        float *line, int64_t line_channel_pitch, int form, void *stream);

/* ---- Detection mask (cube_detect.hip): the pieces of a smooth-and-clip source finder on a spectral
 * cube (SoFiA's S+C finder, the masks built by hand around CASA immoments, tclean's auto-multithresh
 * on cubes): the cube is smoothed with a set of spatial and spectral kernels, each smoothed copy is
 * thresholded at a multiple of its own measured noise, and the union is the detection mask.  The
 * spatial smoothing is kimg_cube_smooth's and the noise kimg_cube_stats'; here are the spectral
 * boxcar, the restoring of blanks, the threshold into the mask, the pruning of short runs and the
 * mask applied to a cube, which is how kimg_moments honours it (NaN is "not usable" there already).
 * The reference has none; the semantics are this library's, and katsdpimager_amd/detect.py holds them
 * once more as numpy (boxcar_host, reblank_host, threshold_host, prune_host, apply_host) together with
 * the finder's order of calls (smooth_clip_host).
 *
 * Shared by the five entries.  A cube is DEVICE float32 [C][M]: C = num_channels (1 ..
 *   KIMG_MOMENTS_MAX_CHANNELS) planes of M = plane_elements values (for images [P][H][W], dense,
 *   M = P * H * W), a channel pitch in elements apart, pitch >= M, as in kimg_moments; every cube of a
 *   call has a pitch of its own.  The mask is DEVICE uint8 [C][M], mask_pitch in bytes >= M: 0 = not
 *   detected, 1 = detected; the kernels write only 0 or 1 and read any nonzero value as set.
 *   filled_host: HOST uint8 [C], nonzero = the plane holds an image; it is read during the call and
 *   travels by value, a bit per channel.  Padding is neither read nor written.  Indices are 64-bit.
 *   "Not finite" is NaN of any sign or payload, +Inf and -Inf.
 * Load forms, as in kimg_moments: four elements per thread with 16-byte float accesses where every
 *   float base and pitch * 4 of the call is 16-byte aligned, for the first 4 * (M / 4) elements, one
 *   element per thread for the tail and for everything else; with them the mask's four bytes are one
 *   4-byte load where the mask's base and pitch are 4-byte aligned and four byte loads where not.
 *   Bytes of the mask are STORED one by one, only where the contract names them.  kimg_cube_reblank
 *   and kimg_cube_threshold store single elements, so only their loads have the 16-byte form, and
 *   kimg_cube_mask_prune's four-wide form needs the mask's 4-byte alignment alone.
 * Returns, before any HIP call: KIMG_EINVAL for a null pointer (kimg_cube_boxcar's mask excepted), C < 1,
 *   M < 0 (kimg_cube_threshold: P, H or W below 1), a float pointer that is not 4-byte aligned, a
 *   pitch below M, and what an entry lists below; KIMG_EUNSUPPORTED for C > KIMG_MOMENTS_MAX_CHANNELS
 *   or M beyond the grid limit (2^31 - 1 workgroups of 256 elements; kimg_cube_boxcar: of 64).  M = 0
 *   is then a successful call that does nothing.
 * Asynchronous on `stream`, no allocation, no workspace, capturable; equal inputs give equal bits.
 * Agreement with the twins: bit for bit, NaN in the same places.  Everything is exact selection, one
 *   named float32 operation, or a float64 sum in a stated order in a build that fuses nothing.
 *
 * kimg_cube_boxcar: the spectral boxcar with replacement.  width = w = 2 h + 1, odd, 1 ..
 *   KIMG_BOXCAR_MAX_WIDTH.  Per element m on its own: for a channel c', z[c'] = cube[c'][m] iff
 *   0 <= c' < C, filled[c'], the value is finite and (mask is NULL or mask[c'][m] == 0); else +0.0f.
 *   For every filled c, in float64, nothing fused, c' ascending from c - h to c + h:
 *       acc = 0.0;  acc = acc + (double) z[c']
 *   and out[c][m] = (float) (acc / (double) w): always divided by w, which is zero padding at the ends
 *   of the band.  With blank != 0, out[c][m] = 0x7fc00000 where cube[c][m] itself is not finite.
 *   Channels that are not filled are not written.  out shares no byte with the cube (KIMG_EINVAL; in
 *   place is not done).  width = 1 is the copy with non-finite and already-detected voxels made 0.
 *   The sum is a direct one: a running add-and-subtract window does not have its bits and is not
 *   what this is.  Also KIMG_EINVAL: an even width, one outside 1 .. 31.
 *   Kernel: a workgroup of one wave keeps the last w + 6 channels of its elements in LDS (8 .. 64
 *   rows of 1 KiB at four elements per thread); every voxel is read from memory once whatever w is.
 * kimg_cube_reblank: for every filled c, work[c][m] = 0x7fc00000 where cube[c][m] is not finite;
 *   nothing else is written.  After the spatial smoothing of a boxcar's result (whose blanks were
 *   made 0), it keeps blanked voxels out of the noise and the threshold.  work shares no byte with
 *   the cube (KIMG_EINVAL).
 * kimg_cube_threshold: sigma is DEVICE float32 [C][groups], what kimg_cube_stats wrote; groups is 1
 *   (pooled) or P.  Per filled c and element m of polarization p: g = groups == 1 ? 0 : p,
 *   cut = threshold * sigma[c * groups + g] (one float32 product), s = work[c][m].  The voxel is
 *   detected iff s is finite and, in a float32 compare, s > cut (KIMG_DETECT_POSITIVE), -s > cut
 *   (KIMG_DETECT_NEGATIVE) or fabsf(s) > cut (KIMG_DETECT_BOTH); a NaN cut detects nothing.  A detected
 *   voxel sets mask[c][m] = 1; nothing else of the mask is written and nothing is ever cleared.  The
 *   host does not read sigma.  Also KIMG_EINVAL: groups other than 1 and P, a threshold that is not a
 *   finite number above 0, an unknown polarity, a sigma that is not 4-byte aligned.
 * kimg_cube_mask_prune: per element m, every maximal run of consecutive channels with a nonzero mask
 *   that is shorter than min_channels (1 .. C) is cleared to 0, and a nonzero byte of a run that stays
 *   becomes 1.  All C channels are walked: a channel that is not filled is one whose mask is 0.  With
 *   min_channels = 1 nothing is cleared, and a mask of 0 and 1 is left as it is.  Also KIMG_EINVAL:
 *   min_channels outside 1 .. C.
 * kimg_cube_mask_apply: for every filled c, line[c][m] = cube[c][m] where
 *   (mask[c][m] != 0) != (invert != 0), else 0x7fc00000.  line is either exactly `cube` (the same
 *   pointer AND the same pitch: in place) or shares no byte with it (kimg_spectrum_stats' rule;
 *   KIMG_EINVAL).  Channels that are not filled are neither read nor written.
 *
 * Not done here (linking the mask into sources and a catalogue is "Source linking" below):
 *   reliability from negative detections; mask dilation; a running-window boxcar; the noise of a
 *   smoothed cube derived rather than measured; spatial kernels beyond radius 16; kimg_moments reading
 *   the mask itself; cubes across several GPUs. */
#define KIMG_BOXCAR_MAX_WIDTH 31
#define KIMG_DETECT_POSITIVE 0
#define KIMG_DETECT_NEGATIVE 1
#define KIMG_DETECT_BOTH 2
int kimg_cube_boxcar(const float *cube, int64_t channel_pitch, const uint8_t *mask, int64_t mask_pitch,
                     float *out, int64_t out_channel_pitch, int num_channels, int64_t plane_elements,
                     const uint8_t *filled_host, int width, int blank, void *stream);
int kimg_cube_reblank(float *work, int64_t work_channel_pitch, const float *cube,
                      int64_t channel_pitch, int num_channels, int64_t plane_elements,
                      const uint8_t *filled_host, void *stream);
int kimg_cube_threshold(const float *work, int64_t work_channel_pitch, uint8_t *mask,
                        int64_t mask_pitch, int num_channels, int num_polarizations, int height,
                        int width, const uint8_t *filled_host, const float *sigma, int groups,
                        float threshold, int polarity, void *stream);
int kimg_cube_mask_prune(uint8_t *mask, int64_t mask_pitch, int num_channels, int64_t plane_elements,
                         int min_channels, void *stream);
int kimg_cube_mask_apply(const float *cube, int64_t channel_pitch, const uint8_t *mask,
                         int64_t mask_pitch, float *line, int64_t line_channel_pitch,
                         int num_channels, int64_t plane_elements, const uint8_t *filled_host,
                         int invert, void *stream);

/* ---- Source linking (cube_link.hip): the detection mask linked into sources -- which voxels belong
 * together, how many sources there are, where each one is and how bright -- measured into a catalogue,
 * filtered by size, and handed back as a mask (SoFiA's linker and parameteriser, the seeds of CASA's
 * imfit, the region list that immoments takes per source).  The reference has none; the semantics are
 * this library's, and katsdpimager_amd/link.py holds them once more as numpy (link_host, measure_host,
 * filter_host, label_mask_host).
 *
 * Shared by the entries.  The mask is DEVICE uint8 [C][M] with mask_pitch in bytes, the labels DEVICE
 *   int32 [C][M] with a pitch of their own in elements, the cube DEVICE float32 [C][M] with its own
 *   pitch; every pitch >= M; M = P * H * W, dense, as in kimg_cube_threshold.  filled_host: HOST uint8
 *   [C], read during the call, travels by value.  A voxel is SET iff its channel is filled and its
 *   mask byte is nonzero; unfilled channels of the mask and of the cube are not read.  d(c, m) =
 *   c * M + m is the DENSE INDEX of a voxel; it knows no pitch, and nothing in a result depends on a
 *   pitch, an offset or the launch geometry.  Padding is neither read nor written.
 * Neighbours: two set voxels (c, p, y, x) and (c', p', y', x') iff p == p', |c - c'| <= reach_z
 *   (0 .. 3) and (x - x')^2 + (y - y')^2 <= reach_xy_sq (0 .. 9).  The channel distance counts
 *   channels, filled or not.  Polarization is never a linking axis.  A source is a connected
 *   component of this relation.
 *
 * kimg_cube_link: labels[c][m] = 0 for a voxel that is not set (in every channel, filled or not: the
 *   whole label cube is written), else the number of its source, 1 .. N0, sources numbered in
 *   ascending order of their smallest dense index; counts[0] = N0 (counts: DEVICE int32 [2]).  For
 *   reach_xy_sq in {1, 2} and reach_z <= 1 this is scipy.ndimage.label on [C][P][H][W] with a
 *   structure that is empty along P.  Integers only: the same bits on every run.
 *   Kernel: a lock-free union-find in the label cube (the smaller dense index is the root, atomicMin,
 *   relaxed agent-scope loads), six launches: init, merge, flatten with a count of roots per
 *   workgroup, a scan of those counts, the roots numbered, every voxel relabelled.
 *   scratch: DEVICE, kimg_cube_link_scratch_bytes(C, M) bytes (0 for arguments out of range), 4-byte
 *   aligned; the call initialises it.
 * kimg_catalogue: a HOST struct of DEVICE arrays [capacity] each, read during the call; row s - 1 is
 *   source s.  work: kimg_cube_catalogue_work_bytes(capacity) bytes, 8-byte aligned, the calls' own.
 * kimg_cube_measure: for every source s <= min(counts[0], capacity), over the voxels of filled
 *   channels with labels[c][m] == s: first = the smallest dense index; voxels = their number; finite =
 *   the number whose cube value is finite; the inclusive bounding box c0, c1, y0, y1, x0, x1.  Over
 *   the finite ones: peak = the largest value in kimg_cube_stats' order (key(x) of the bit pattern, -0
 *   below +0) and peak_index its dense index, the smallest on ties; trough and trough_index likewise
 *   for the smallest value; NaN (0x7fc00000) and -1 where finite == 0.  sum = sum f, sum_c = sum f * c,
 *   sum_y = sum f * y, sum_x = sum f * x: float64, nothing fused, one product per term, c, y, x exact
 *   doubles, 0 where finite == 0.  Rows beyond counts[0] and sources beyond capacity are not written.
 *   The integer and peak fields are exact.  The ORDER of the four sums is not part of the contract
 *   (they are float64 atomic adds of per-thread partial sums): on values whose sums are exact in
 *   every order they equal the twin's, otherwise each differs from the exactly rounded sum by at
 *   most n * 2^-53 * sum |term|, n = finite.
 *   Kernel: a thread owns four consecutive elements of the plane for the whole channel loop and keeps
 *   the partial sums, counts, box and keys of the current run of equal labels in registers; it issues
 *   its atomics when the label changes or the walk ends.  Peaks are a 64-bit atomicMax on (value key,
 *   inverted dense index), decoded by a last small launch.
 * kimg_cube_link_filter: with N0 = counts[0] <= capacity, a source is kept iff voxels >= min_voxels,
 *   x1 - x0 + 1 >= min_size_xy, y1 - y0 + 1 >= min_size_xy and c1 - c0 + 1 >= min_size_z.  Kept
 *   sources are renumbered 1 .. N in their old order, their rows compacted to the front (rows N ..
 *   N0 - 1 keep what they held), every label rewritten (dropped sources become 0), counts[1] = N.
 *   With all three minima at 1 nothing changes.  With N0 > capacity nothing is changed at all and
 *   counts[1] = N0.  Takes (C, M); no mask, no cube, no filled.
 * kimg_cube_label_mask: mask[c][m] = 1 where labels[c][m] != 0 (source == 0) or labels[c][m] ==
 *   source (source > 0), else 0, in every channel: the whole mask is written.
 *
 * Returns, before any HIP call: KIMG_EINVAL for a null pointer, C < 1, P, H or W below 1 (M < 0 where
 *   an entry takes M), a pitch below M, a labels, cube, counts or scratch pointer that is not 4-byte
 *   aligned, a reach out of range, capacity < 1, a catalogue with a null or misaligned array (4 bytes;
 *   the sums and work 8), a minimum below 1, a source below 0; then KIMG_EUNSUPPORTED for
 *   C > KIMG_MOMENTS_MAX_CHANNELS or C * M > 2^31 - 2 (labels are int32).  M = 0 is then a successful
 *   call that does nothing to cubes.
 * Asynchronous on `stream`, no allocation, capturable; the host reads nothing.
 * Not done here (per-source spectra, fluxes in Jy and their errors are "Source spectra and line
 *   parameters" below, the moment maps of every source "Per-source moment maps"): reliability from
 *   negative detections; mask dilation; sources across polarizations; cubes across
 *   several GPUs; bit-reproducible sums (a store-and-sum pass, another contract). */
typedef struct kimg_catalogue {
    int32_t *first, *voxels, *finite, *c0, *c1, *y0, *y1, *x0, *x1;
    float *peak;
    int32_t *peak_index;
    float *trough;
    int32_t *trough_index;
    double *sum, *sum_c, *sum_y, *sum_x;
    void *work;
} kimg_catalogue;
size_t kimg_cube_link_scratch_bytes(int num_channels, int64_t plane_elements);
size_t kimg_cube_catalogue_work_bytes(int capacity);
int kimg_cube_link(const uint8_t *mask, int64_t mask_pitch, int32_t *labels, int64_t label_pitch,
                   int num_channels, int num_polarizations, int height, int width,
                   const uint8_t *filled_host, int reach_xy_sq, int reach_z, void *scratch,
                   int32_t *counts, void *stream);
int kimg_cube_measure(const int32_t *labels, int64_t label_pitch, const float *cube,
                      int64_t channel_pitch, int num_channels, int num_polarizations, int height,
                      int width, const uint8_t *filled_host, const kimg_catalogue *catalogue,
                      int capacity, const int32_t *counts, void *stream);
int kimg_cube_link_filter(int32_t *labels, int64_t label_pitch, int num_channels,
                          int64_t plane_elements, const kimg_catalogue *catalogue, int capacity,
                          int min_voxels, int min_size_xy, int min_size_z, int32_t *counts,
                          void *stream);
int kimg_cube_label_mask(const int32_t *labels, int64_t label_pitch, uint8_t *mask, int64_t mask_pitch,
                         int num_channels, int64_t plane_elements, int source, void *stream);

/* ---- Source spectra and line parameters (cube_sources.hip): what a source finder ends with (SoFiA's
 * parameteriser) -- the integrated spectrum of every linked source, and from it the flux with its
 * error, the peak flux density, the centroid and the line widths w50 and w20.  The reference has none;
 * the semantics are this library's, and katsdpimager_amd/sources.py holds them once more as numpy
 * (source_spectra_host, source_lines_host).
 *
 * The ragged layout, shared by the two entries.  num_sources = N: sources 1 .. N.  c0: DEVICE int32
 *   [N], the first channel of each source's range.  offsets: DEVICE int32 [N + 1].  Source s owns the
 *   entries offsets[s-1] .. offsets[s] - 1 of every table, one per channel c0[s-1] + k.  total =
 *   offsets[N] <= 2^31 - 2 is the length of every table.  (The ranges are the caller's: the
 *   catalogue's c0 .. c1 of kimg_cube_measure, or wider.)  c0 and offsets are DEVICE data that the host
 *   cannot check, so the kernels do: see below.
 *
 * kimg_cube_source_spectra: labels, label_pitch, cube, channel_pitch, C = num_channels, M =
 *   plane_elements, filled_host, the dense index, the pitches and "unfilled channels are not read,
 *   padding is neither read nor written" are those of "Source linking" above.  sum: DEVICE float64
 *   [total]; voxels, finite: DEVICE int32 [total].  The call first zeroes all `total` entries of the
 *   three tables.  Then, for every source s and channel c of its range, over the voxels of channel c
 *   (filled) with labels[c][m] == s: voxels = their number, finite = the number whose cube value is
 *   finite, sum = the float64 sum of the finite values.  Entries of unfilled channels inside a range
 *   therefore read 0.  A voxel whose label is <= 0 or > N, or whose channel lies outside its row's
 *   [c0, c0 + offsets[s] - offsets[s-1]), is skipped; an entry is written only at an index inside
 *   both its row and [0, total), so that wrong c0 or offsets give wrong numbers, never a write outside
 *   the tables.  The two counts are exact.  The ORDER of the sum is not part of the contract (float64
 *   atomic adds of partial sums, as kimg_cube_measure's): on values whose sums are exact in every
 *   order it equals the twin's (which sums in ascending dense index), otherwise it differs from the
 *   exactly rounded sum by at most n * 2^-53 * sum |term|, n = finite.
 *   Kernel: one read of labels and cube, 16-byte loads where base and pitch allow; within a wave the
 *   lanes that hold the same label in consecutive lanes combine their sums and counts by shuffles
 *   before one lane issues the atomics.
 *   Returns, before any HIP call: KIMG_EINVAL for a null pointer, a pointer that is not 4-byte (sum:
 *   8-byte) aligned, N < 0, total < 0, C < 1, M < 0, a pitch below M; then KIMG_EUNSUPPORTED for
 *   C > KIMG_MOMENTS_MAX_CHANNELS, C * M > 2^31 - 2 or total > 2^31 - 2.  N = 0 or M = 0 is then a
 *   successful call that writes nothing.  Asynchronous on `stream`, no allocation, capturable; the host
 *   reads nothing.
 *
 * kimg_source_lines: N, c0, offsets, total as above; sum, finite: the tables of
 *   kimg_cube_source_spectra (read only).  C = num_channels.  unit_host, width_host, coord_host,
 *   variance_host: HOST float64 [C], read during the call: the entry copies them on `stream` into
 *   channel_tables, DEVICE float64 [4 * C], 8-byte aligned, the caller's space (so the call is
 *   asynchronous but, for these copies, not capturable).  unit[c] turns a sum of pixel values into a
 *   flux density (1 / beam area in pixels for Jy/beam), width[c] is the channel's width on the axis
 *   of coord[c], variance[c] the variance that ONE finite voxel of channel c adds to the flux.
 *   lines: a HOST struct of DEVICE arrays [N] each, row s - 1 is source s.
 *   One thread per source; everything float64, in ascending channel order, nothing fused, one product
 *   per term.  With n = offsets[s] - offsets[s-1], k = 0 .. n - 1, c = c0[s-1] + k, d_k = sum_k *
 *   unit[c], x_k = coord[c]:
 *     flux:     F = 0; F = F + d_k * width[c].
 *     flux_err: V = 0; V = V + (double) finite_k * variance[c]; flux_err = sqrt(V).
 *     peak, peak_channel: over the entries with finite_k > 0 in ascending k, the first d_k, replaced
 *               only by a d_k > peak (the lowest channel wins a tie); peak_channel = c0 + k of it.  NaN
 *               and -1 without such an entry.
 *     centroid: S0 = 0, S1 = 0; S0 = S0 + d_k; S1 = S1 + d_k * x_k; centroid = S1 / S0, NaN where
 *               S0 == 0.
 *     w50, w20 (SoFiA's rule), only where peak > 0, NaN otherwise: L = 0.5 * peak (0.2 * peak).  k =
 *               the first entry from the low end with d_k >= L; lo = x_0 if k == 0, else
 *               x_{k-1} + (((L - d_{k-1}) / (d_k - d_{k-1})) * (x_k - x_{k-1})).  k = the first entry
 *               from the high end with d_k >= L; hi = x_{n-1} if k == n - 1, else
 *               x_{k+1} + (((L - d_{k+1}) / (d_k - d_{k+1})) * (x_k - x_{k+1})).  w = |hi - lo|.  The
 *               edges are outputs too: w50_lo, w50_hi, w20_lo, w20_hi.
 *     channels = n.
 *   Every NaN that is written is 0x7ff8000000000000.  The float64 divide and sqrt of this build are
 *   correctly rounded, so given the same spectra the device has the twin's bits.  A row whose range
 *   leaves 0 .. C or whose entries leave 0 .. total is treated as one with n = 0 (flux 0, error 0,
 *   the rest NaN / -1): nothing outside the tables is read.
 *   Returns, before any HIP call: KIMG_EINVAL for a null pointer, a misaligned one (4 bytes; 8 for
 *   float64), a lines struct with a null or misaligned array, N < 0, total < 0, C < 1; then
 *   KIMG_EUNSUPPORTED for C > KIMG_MOMENTS_MAX_CHANNELS or total > 2^31 - 2.  N = 0 is then a
 *   successful call that copies and writes nothing.
 *
 * Not done here (per-source moment maps, whose sums are bit-reproducible, are "Per-source moment maps"
 *   below): reliability from negative detections; mask dilation; bit-reproducible sums of the spectra
 *   (a store-and-sum pass, another contract); sources across polarizations;
 *   Gaussian or busy-function fits to the spectra; cubes across several GPUs. */
typedef struct kimg_source_line_table {
    double *flux, *flux_err, *peak;
    int32_t *peak_channel;
    double *centroid, *w50, *w20, *w50_lo, *w50_hi, *w20_lo, *w20_hi;
    int32_t *channels;
} kimg_source_line_table;
int kimg_cube_source_spectra(const int32_t *labels, int64_t label_pitch, const float *cube,
                             int64_t channel_pitch, int num_channels, int64_t plane_elements,
                             const uint8_t *filled_host, int num_sources, const int32_t *c0,
                             const int32_t *offsets, int64_t total, double *sum, int32_t *voxels,
                             int32_t *finite, void *stream);
int kimg_source_lines(int num_sources, const int32_t *c0, const int32_t *offsets, int64_t total,
                      const double *sum, const int32_t *finite, int num_channels,
                      const double *unit_host, const double *width_host, const double *coord_host,
                      const double *variance_host, double *channel_tables,
                      const kimg_source_line_table *lines, void *stream);

/* ---- Per-source moment maps (cube_source_maps.hip): the moment maps of EVERY linked source inside its
 * own bounding box, in one pass over labels and cube -- what SoFiA writes next to its catalogue and
 * what immoments gives per region.  The reference has none; the semantics are this library's, and
 * katsdpimager_amd/source_maps.py holds them once more as numpy (source_maps_host).
 *
 * Inputs.  labels: DEVICE int32 [C][P][H][W], label_pitch elements from channel to channel; cube:
 *   DEVICE float32 of the same shape with a pitch of its own; both pitches >= P * H * W, the [P][H][W]
 *   plane dense, padding neither read nor written; neither array is ever written.  filled_host: HOST
 *   uint8 [C], read during the call, travels to the kernel by value, a bit per channel.  x: DEVICE
 *   float64 [C], the coordinate of every channel.  rows: DEVICE kimg_source_map_row [N], row s - 1 is
 *   source s (1 .. N = num_sources): offset, pol, the box's corner y0, x0 and its extent h, w, the
 *   channel range c0 .. c1 (inclusive), and x_ref and width of "Moment maps" for that range, made by
 *   the host: x_ref = x[(c0 + c1 + 1) / 2], width = |x[c1] - x[c0]| / (c1 - c0), or the channel width
 *   for c0 == c1.  Rows come in ascending offset.
 * The ragged layout.  Source s owns h_s * w_s entries of every table from offset_s on; the entry of
 *   its pixel (y, x) is offset_s + (y - y0_s) * w_s + (x - x0_s).  total <= 2^31 - 2 is the length of
 *   every table; for the rows the host makes, total = offset_N + h_N * w_N.  Boxes of different sources
 *   may overlap in the plane: their entries do not.
 * Which voxels enter.  Voxel (c, p, y, x) with label s enters entry (s, y, x) iff 1 <= s <= N,
 *   filled[c], p == pol_s, 0 <= y - y0_s < h_s, 0 <= x - x0_s < w_s, c0_s <= c <= c1_s, offset_s >= 0
 *   and the entry's index is < total.  Every other voxel is skipped.  The rows are DEVICE data that the
 *   host cannot check, so the kernels do: an index is formed only from a row whose box holds the pixel,
 *   and is checked against total, so that wrong rows give wrong numbers, never an access outside the
 *   tables.  Unfilled channels are not read; the cube is read only where a wave of 64 lanes (256
 *   consecutive plane elements, or 64 in the one-element form) holds a label.
 * Arithmetic.  Per entry, over the voxels that enter in ascending channel order, exactly the sample
 *   rule of "Moment maps" without a cut: only a finite I counts; n += 1; d = x[c] - x_ref_s; S0 += I;
 *   t = I * d; S1 += t; S2 += t * d, float64, nothing fused; the peak (float32, starting at -inf) is
 *   replaced, with its channel, only if I > peak.
 * kimg_cube_source_maps gathers these sums into the state table in `workspace` (8-byte aligned, at
 *   least kimg_cube_source_maps_workspace_bytes(total) = 36 * total bytes, zeroed by the call with a
 *   hipMemsetAsync): a column walk, one thread per pixel (four consecutive plane elements per thread
 *   with 16-byte label and cube loads where labels, cube and both pitches * 4 are 16-byte aligned, for
 *   the first 4 * (M / 4) elements; one element per thread for the tail and everything else).  A
 *   thread keeps the sums of the source at its pixel in registers and exchanges them with the state
 *   table, by plain stores and loads, only where the label at the pixel changes to another source's.  No
 *   atomics, so equal inputs give equal bits.
 * kimg_source_maps_finish turns the state into the tables that `outputs` (KIMG_MOMENT_* bits, as in
 *   kimg_moments; the pointer of a bit that is not set is ignored) asks for, float32 [total] each and
 *   count int32 [total], one thread per entry, its source found by binary search in the offsets.  The
 *   formulas are kimg_moments': S0 * width_s; x_ref_s + S1 / S0; sqrt(max(0, S2 / S0 - r * r)); the
 *   peak; x of the peak's channel; NaN where n == 0, moments 1 and 2 also unless S0 > 0.  An entry that
 *   no voxel entered -- a box pixel the source never touches, or an index inside no row's box -- reads
 *   NaN and count 0.  All `total` entries of every requested table are written, and nothing else.
 * Agreement.  Entry (s, y, x) equals, bit for bit and moment 2 included, what kimg_moments gives at
 *   (pol_s, y, x) over first = c0_s, stop = c1_s + 1 with cut -inf on the cube with every voxel not
 *   labelled s set to NaN: both units compile the same expressions (csrc/kimg_moment_math.h).
 * Returns, before any HIP call: KIMG_EINVAL for a null or misaligned pointer (4 bytes; 8 for x, rows
 *   and the workspace), C, P, H or W below 1, N < 0, total < 0, a pitch below P * H * W, outputs without
 *   any KIMG_MOMENT_* bit or with others, or a requested output that is NULL; then KIMG_EUNSUPPORTED for
 *   C > KIMG_MOMENTS_MAX_CHANNELS, C * P * H * W > 2^31 - 2 or total > 2^31 - 2; then KIMG_EWORKSPACE for
 *   a short workspace.  N = 0 or total = 0 is then a successful call that does nothing.  Asynchronous on
 *   `stream`, no allocation; the host reads nothing.
 * Not done here: pasting the maps back into one plane; a noise cut or Hanning selection per source;
 *   sources across polarizations; cubes across several GPUs. */
typedef struct kimg_source_map_row {
    int32_t offset, pol, y0, x0, h, w, c0, c1;
    double x_ref, width;
} kimg_source_map_row;
size_t kimg_cube_source_maps_workspace_bytes(int64_t total);
int kimg_cube_source_maps(const int32_t *labels, int64_t label_pitch, const float *cube,
                          int64_t channel_pitch, int num_channels, int num_polarizations, int height,
                          int width, const uint8_t *filled_host, const double *x, int num_sources,
                          const kimg_source_map_row *rows, int64_t total, void *workspace,
                          size_t workspace_bytes, void *stream);
int kimg_source_maps_finish(int num_sources, const kimg_source_map_row *rows, int64_t total,
                            const void *workspace, size_t workspace_bytes, const double *x,
                            int num_channels, int outputs, float *moment0, float *moment1,
                            float *moment2, float *moment8, float *moment9, int32_t *count,
                            void *stream);

#ifdef __cplusplus
}
#endif
#endif /* KIMG_H */
