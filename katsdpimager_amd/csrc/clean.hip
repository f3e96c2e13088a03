// Hogbom CLEAN kernels: per-tile peak, global peak, PSF subtract, PSF patch bound, the
// radix-select passes of the noise estimate, and a device-resident minor-cycle loop.
// Mirrors clean.py:123-163, 295-353, 451-480, 566-587, 683-726, 848-891 of the reference.
//
// Peak selection is BIT-EXACT with the reference host path (CleanHost, clean.py:946-1075):
//  - within a tile: first strict maximum in row-major order (clean.py:953-958), and a tile
//    with no positive metric keeps value 0 and the (x0, y0) initial position (clean.py:950);
//  - across tiles: first maximum in row-major tile order (np.argmax, clean.py:1062);
//  - subtraction is dirty -= (loop_gain*pixel) * psf with separately rounded multiply and
//    subtract (clean.py:1044-1046): this file is built with -ffp-contract=off.
#include "kimg_common.h"
#include "kimg_graph_cache.h"
#include "kimg_peak_key.h"
#include <limits.h>
#include <string.h>

namespace {

constexpr int TILE = 32;            // clean.py:996

template <int MODE>
__device__ inline float clean_metric(const float *__restrict__ dirty, int64_t addr,
                                     int64_t pol_stride, int P)
{
    if (MODE == KIMG_CLEAN_I)
        return fabsf(dirty[addr]);
    float value = 0.0f;                                // clean.py:962-964
    for (int p = 0; p < P; p++) {
        float pix = dirty[addr + p * pol_stride];
        value += pix * pix;
    }
    return value;
}

// Scan tile (tx, ty): pixels [x0,x1) x [y0,y1); 256 threads, 4 pixels each in row-major order.
// MASKED: only pixels with a nonzero byte in `mask` (uint8 [height][width], one plane for all
// polarizations, read with the row mapping of the dirty row) are candidates; a tile without any
// records what an all-zero tile records.  Without MASKED the mask arguments are unused (null).
template <int MODE, bool MASKED>
__device__ inline void tile_peak(const float *__restrict__ dirty, int64_t row_stride,
                                 int64_t pol_stride, int width, int height, int P, int border,
                                 int tx, int ty, float *__restrict__ tile_max,
                                 int32_t *__restrict__ tile_pos, int tiles_x,
                                 const uint8_t *__restrict__ mask, int64_t mask_row_stride)
{
    const int x0 = tx * TILE + border, y0 = ty * TILE + border;
    __shared__ key_t s_keys[4];
    key_t b = 0;                        // only positive metrics count (clean.py:953-958)
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int idx = threadIdx.x + k * 256;
        const int x = x0 + (idx & 31), y = y0 + (idx >> 5);
        if (x < width - border && y < height - border
            && (!MASKED || mask[(int64_t) y * mask_row_stride + x])) {
            float v = clean_metric<MODE>(dirty, (int64_t) y * row_stride + x, pol_stride, P);
            if (v > 0.0f)
                b = key_max(b, make_key(v, idx));
        }
    }
    b = block_max_key(b, s_keys);
    if (threadIdx.x == 0) {
        const int t = ty * tiles_x + tx;
        store_tile_record(b, x0, y0, tile_max, tile_pos, t);
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void update_tiles_kernel(
    const float *__restrict__ dirty, int64_t row_stride, int64_t pol_stride, int width,
    int height, int P, int border, float *__restrict__ tile_max, int32_t *__restrict__ tile_pos,
    int tiles_x, int tile_x0, int tile_y0)
{
    tile_peak<MODE, false>(dirty, row_stride, pol_stride, width, height, P, border,
                           tile_x0 + blockIdx.x, tile_y0 + blockIdx.y, tile_max, tile_pos, tiles_x,
                           nullptr, 0);
}

template <int MODE>
__global__ __launch_bounds__(256) void update_tiles_masked_kernel(
    const float *__restrict__ dirty, int64_t row_stride, int64_t pol_stride, int width,
    int height, int P, int border, float *__restrict__ tile_max, int32_t *__restrict__ tile_pos,
    int tiles_x, int tile_x0, int tile_y0, const uint8_t *__restrict__ mask,
    int64_t mask_row_stride)
{
    tile_peak<MODE, true>(dirty, row_stride, pol_stride, width, height, P, border,
                          tile_x0 + blockIdx.x, tile_y0 + blockIdx.y, tile_max, tile_pos, tiles_x,
                          mask, mask_row_stride);
}

// Global argmax over tiles, by a 1024-thread block; every thread returns the winning tile index
// (or -1 when there are no tiles).  All of a thread's loads are issued together and clamped
// instead of predicated (a duplicate of the last tile under a larger index never wins).
__device__ inline int peak_tile(const float *__restrict__ tile_max, int num_tiles, float &value)
{
    __shared__ key_t s_peak[16];
    key_t best = 0;
    constexpr int ROUND = 16;
    for (int base = threadIdx.x; base < num_tiles; base += ROUND * blockDim.x) {
        float v[ROUND];
#pragma unroll
        for (int k = 0; k < ROUND; k++)
            v[k] = tile_max[min(base + k * (int) blockDim.x, num_tiles - 1)];
        key_t c[ROUND];
#pragma unroll
        for (int k = 0; k < ROUND; k++)
            c[k] = make_key(v[k], base + k * (int) blockDim.x);
#pragma unroll
        for (int w = ROUND / 2; w > 0; w >>= 1)
#pragma unroll
            for (int k = 0; k < w; k++)
                c[k] = key_max(c[k], c[k + w]);
        best = key_max(best, c[0]);
    }
    best = block_max_key(best, s_peak);
    value = best ? __uint_as_float((unsigned) (best >> 32)) : -1.0f;
    return best ? ~(int) (unsigned) best : -1;
}

// MASKED: a best metric of exactly 0 means that no allowed pixel is left to take (the winning
// record would be the (x0, y0) start position of a tile without candidates, which may be a masked
// pixel): the search ends, reported as position (-1, -1) with a zero pixel.
template <bool MASKED>
__device__ inline void find_peak(
    const float *__restrict__ dirty, int64_t row_stride, int64_t pol_stride, int P,
    const float *__restrict__ tile_max, const int32_t *__restrict__ tile_pos, int num_tiles,
    float *__restrict__ peak_value, int32_t *__restrict__ peak_pos, float *__restrict__ peak_pixel)
{
    float value;
    int t = peak_tile(tile_max, num_tiles, value);
    if (MASKED && threadIdx.x == 0 && t >= 0 && value == 0.0f) {
        *peak_value = 0.0f;
        peak_pos[0] = -1;
        peak_pos[1] = -1;
        for (int p = 0; p < P; p++)
            peak_pixel[p] = 0.0f;
        return;
    }
    if (threadIdx.x == 0 && t >= 0) {
        const int y = tile_pos[2 * t], x = tile_pos[2 * t + 1];
        *peak_value = value;
        peak_pos[0] = y;
        peak_pos[1] = x;
        for (int p = 0; p < P; p++)
            peak_pixel[p] = dirty[p * pol_stride + (int64_t) y * row_stride + x];
    }
}

__global__ __launch_bounds__(1024) void find_peak_kernel(
    const float *__restrict__ dirty, int64_t row_stride, int64_t pol_stride, int P,
    const float *__restrict__ tile_max, const int32_t *__restrict__ tile_pos, int num_tiles,
    float *__restrict__ peak_value, int32_t *__restrict__ peak_pos, float *__restrict__ peak_pixel)
{
    find_peak<false>(dirty, row_stride, pol_stride, P, tile_max, tile_pos, num_tiles, peak_value,
                     peak_pos, peak_pixel);
}

__global__ __launch_bounds__(1024) void find_peak_masked_kernel(
    const float *__restrict__ dirty, int64_t row_stride, int64_t pol_stride, int P,
    const float *__restrict__ tile_max, const int32_t *__restrict__ tile_pos, int num_tiles,
    float *__restrict__ peak_value, int32_t *__restrict__ peak_pos, float *__restrict__ peak_pixel)
{
    find_peak<true>(dirty, row_stride, pol_stride, P, tile_max, tile_pos, num_tiles, peak_value,
                    peak_pos, peak_pixel);
}

struct pixel_t { float v[4]; };

__global__ __launch_bounds__(256) void subtract_psf_kernel(
    float *__restrict__ dirty, float *__restrict__ model, int64_t row_stride, int64_t pol_stride,
    int width, int height, int P, const float *__restrict__ psf, int64_t psf_row_stride,
    int64_t psf_pol_stride, int psf_x0, int psf_y0, int patch_w, int patch_h,
    const float *__restrict__ peak_pixel, int pos_x, int pos_y, int start_x, int start_y,
    float loop_gain)
{
    const int gx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int gy = blockIdx.y * 4 + (threadIdx.x >> 6);
    float scale[4];
    for (int p = 0; p < P; p++)
        scale[p] = loop_gain * peak_pixel[p];
    if (gx == 0 && gy == 0)
        for (int p = 0; p < P; p++)
            model[p * pol_stride + (int64_t) pos_y * row_stride + pos_x] += scale[p];
    if (gx >= patch_w || gy >= patch_h)
        return;
    const int x = start_x + gx, y = start_y + gy;
    if (x < 0 || x >= width || y < 0 || y >= height)
        return;
    const int64_t pa = (int64_t) (psf_y0 + gy) * psf_row_stride + (psf_x0 + gx);
    const int64_t ia = (int64_t) y * row_stride + x;
    for (int p = 0; p < P; p++) {
        const float t = scale[p] * psf[p * psf_pol_stride + pa];
        dirty[p * pol_stride + ia] -= t;
    }
}

// ---- device-resident minor cycles ------------------------------------------------------
struct clean_state {
    int count;          // cycles completed
    int done;           // threshold reached (or `limit` cycles done)
    int limit;          // maximum number of cycles for this call
    float threshold;    // stop when the peak metric falls below it (kept here, not in the kernel
                        // arguments, so that one captured graph serves every threshold)
    int pos_y, pos_x;
    int pad[2];
    float scale[4];     // loop_gain * pixel at the current peak
};

// MASKED: a best metric of exactly 0 ends the loop whatever the threshold (see find_peak).
template <bool MASKED>
__device__ __attribute__((always_inline)) inline void cycle_find_peak(
    const float *__restrict__ dirty, float *__restrict__ model, int64_t row_stride,
    int64_t pol_stride, int P, const float *__restrict__ tile_max,
    const int32_t *__restrict__ tile_pos, int num_tiles, float loop_gain,
    clean_state *__restrict__ state, float *__restrict__ log)
{
    // The kernel is a chain of dependent memory round trips; keep it short: the state words are
    // fetched together with the tile maxima (not before them), and the pixel and model values of
    // all polarizations are fetched together before anything is stored.
    const int4 st = *reinterpret_cast<const int4 *>(state);    // count, done, limit, threshold
    const int count = st.x, done = st.y, limit = st.z;
    const float threshold = __int_as_float(st.w);
    float value;
    const int t = peak_tile(tile_max, num_tiles, value);
    const int p = threadIdx.x;          // one thread per polarization from here on
    if (p >= P || done)
        return;
    if (t < 0 || value < threshold || count >= limit || (MASKED && value == 0.0f)) {   // clean.py:1065-1066
        if (p == 0)
            state->done = 1;
        return;
    }
    const int2 pos = *reinterpret_cast<const int2 *>(tile_pos + 2 * t);
    const int y = pos.x, x = pos.y;
    const int64_t a = p * pol_stride + (int64_t) y * row_stride + x;
    const float pix = dirty[a], mod = model[a];
    float *entry = log + (int64_t) count * (3 + P);
    const float s = loop_gain * pix;            // clean.py:1044
    state->scale[p] = s;
    entry[3 + p] = s;
    model[a] = mod + s;                         // clean.py:1047
    if (p == 0) {
        entry[0] = value;
        entry[1] = __int_as_float(y);
        entry[2] = __int_as_float(x);
        state->pos_y = y;
        state->pos_x = x;
        state->count = count + 1;
    }
}

template <int MODE>
__global__ __launch_bounds__(1024) void cycle_find_peak_kernel(
    const float *__restrict__ dirty, float *__restrict__ model, int64_t row_stride,
    int64_t pol_stride, int P, const float *__restrict__ tile_max,
    const int32_t *__restrict__ tile_pos, int num_tiles, float loop_gain,
    clean_state *__restrict__ state, float *__restrict__ log)
{
    cycle_find_peak<false>(dirty, model, row_stride, pol_stride, P, tile_max, tile_pos, num_tiles,
                           loop_gain, state, log);
}

// (does not depend on the mode: one instantiation serves both)
__global__ __launch_bounds__(1024) void cycle_find_peak_masked_kernel(
    const float *__restrict__ dirty, float *__restrict__ model, int64_t row_stride,
    int64_t pol_stride, int P, const float *__restrict__ tile_max,
    const int32_t *__restrict__ tile_pos, int num_tiles, float loop_gain,
    clean_state *__restrict__ state, float *__restrict__ log)
{
    cycle_find_peak<true>(dirty, model, row_stride, pol_stride, P, tile_max, tile_pos, num_tiles,
                          loop_gain, state, log);
}

// One workgroup per 32x32 block of the tile lattice that the PSF patch can touch: subtract
// the scaled PSF from the block's pixels that lie in the patch, then (if the block is a real
// tile) rescan the tile.  Fuses _subtract_psf + _update_tile of clean.py:1067-1074.
// MASKED form: the subtraction is the same (masked pixels included); only allowed pixels are
// candidates of the rescan (see tile_peak).
template <int MODE>
__global__ __launch_bounds__(256) void cycle_subtract_update_kernel(
    float *__restrict__ dirty, int64_t row_stride, int64_t pol_stride, int width, int height,
    int P, const float *__restrict__ psf, int64_t psf_row_stride, int64_t psf_pol_stride,
    int psf_w, int psf_h, int patch_w, int patch_h, int border,
    float *__restrict__ tile_max, int32_t *__restrict__ tile_pos, int tiles_x, int tiles_y,
    const clean_state *__restrict__ state)
{
#define KIMG_LOAD_ALLOWED(y, x)
#define KIMG_AND_ALLOWED(y, x)
#include "clean_subtract_update.inc"
#undef KIMG_LOAD_ALLOWED
#undef KIMG_AND_ALLOWED
}

template <int MODE>
__global__ __launch_bounds__(256) void cycle_subtract_update_masked_kernel(
    float *__restrict__ dirty, int64_t row_stride, int64_t pol_stride, int width, int height,
    int P, const float *__restrict__ psf, int64_t psf_row_stride, int64_t psf_pol_stride,
    int psf_w, int psf_h, int patch_w, int patch_h, int border,
    float *__restrict__ tile_max, int32_t *__restrict__ tile_pos, int tiles_x, int tiles_y,
    const clean_state *__restrict__ state, const uint8_t *__restrict__ mask,
    int64_t mask_row_stride)
{
#define KIMG_LOAD_ALLOWED(y, x) const bool allowed = mask[(int64_t) (y) * mask_row_stride + (x)] != 0;
#define KIMG_AND_ALLOWED(y, x) && allowed
#include "clean_subtract_update.inc"
#undef KIMG_LOAD_ALLOWED
#undef KIMG_AND_ALLOWED
}

// ---- one launch per minor cycle ----------------------------------------------------------
// The two-launch cycle above is a chain of dependent memory round trips with a kernel boundary
// in the middle.  Here every workgroup of the subtract/update launch finds the global peak
// ITSELF, so the cycle is one launch with no communication between its workgroups.
//
// What a launch needs to know the peak.  Every tile is either one the LAST cycle rewrote -- its new
// record is a "delta": at most (patch / 32 + 2)^2 of them (30 for the 133 x 111 patch of a measured
// PSF), written by the lattice workgroups of the last launch into the slot of their lattice
// position -- or it is not, and the best of THOSE was worked out, off the critical path, during the
// last launch (`rest`).  So a workgroup's first round trip is 48 bytes of state and one delta per
// thread of its first few waves, every candidate arrives with its record (position, pixel values: no
// dependent load), and the peak is one block reduction away: 1.25 us after the first instruction.
// (Rounds 1-2: every workgroup read a 48-byte delta slot and a 16-byte best-two record per THREAD,
// 64 KB, and then fetched its candidate's record: 1.9 us.)
//
// Workgroups of a launch, per channel:
//   * lattice workgroups, one per 32 x 32 block of the tile lattice that the PSF patch can touch:
//     peak, then subtract the PSF from the block, rescan it, and write the new tile record to the
//     OTHER delta table (double-buffered by launch parity), never to the base arrays, so that
//     slower workgroups of the same launch still see the inputs unchanged;
//   * the "keeper": peak, then the log entry, the model pixel, the next state -- and `rest` for the
//     next launch: the best tile outside THIS cycle's lattice, from a table of every owner's best
//     three tiles (thread (b, a) of 1024 owns the tiles with (ty % 32, tx % 32) = (b, a); a patch
//     spans fewer than 32 tiles either way, so a cycle rewrites at most one tile per owner) that is
//     exact up to the cycle before last, plus the last cycle's delta of the owner, if any: three
//     known tiles always decide the best two after one of them changed;
//   * the "folder": folds the last cycle's deltas into the base arrays (plain stores nobody in this
//     launch reads back) and into the owners' table -- a rescan of the 16 (64 at 8192^2) tile maxima
//     of every owner that has one -- written to the OTHER copy of the table, for the next launch's
//     keeper.  Nobody waits for it within the launch.
// The keeper's chain (state + table, peak, candidate, record || reduction, store) and the folder's
// (deltas, rescans, stores) are each about as long as a lattice workgroup's; in round 3's first
// version one workgroup did both and was twice as long as the lattice workgroups (time stamps:
// 6.4 against 3.2 us), which made the cycle slower than before, not faster.
// Tile records carry the pixel values at the tile's peak (tile_pix), which saves the dependent
// load of the peak pixel.  Selection and arithmetic are those of the two-launch form, bit for bit.
constexpr int FUSED_MAX_BLOCKS = 256;     // workgroups of a launch incl. the two bookkeepers: one per CU
constexpr int FUSED_ROUND = 16;           // tile maxima per thread and round of a rescan
constexpr int FUSED_MAX_SLOTS = 4 * FUSED_ROUND;     // 32x32-tile groups: up to 8192^2 pixels

// A tile record rewritten by one cycle and consumed by the next, stored at the slot 32 * (lattice
// row) + (lattice column) of the workgroup that wrote it.  `tag` = 2 + the cycle that wrote it: a
// record is live for exactly the cycle after (0 = never written; the table is cleared per call).
struct __attribute__((aligned(16))) delta_t {
    int tag;
    int tile;
    float value;
    int y, x;
    float pix[4];
    int owner;              // the thread (32 * (ty % 32) + tx % 32) that owns the tile
    int pad[2];
};

struct fused_state {
    int count, done, limit;
    float threshold;
    int pad[12];
};

// The best three tiles among those a thread owns, ordered by (larger value, lower tile index);
// value -1 = none.  Three, because when ONE owned tile gets a new value the owner's best TWO are
// then known without looking at its other tiles (they are no better than the third), and two are
// what the keeper needs: the best tile outside the current cycle's lattice, which holds at most
// one tile of the owner.
struct __attribute__((aligned(16))) owner3_t {
    float v[3];
    int t[3];
    int pad[2];
};
static_assert(sizeof(owner3_t) == 32, "two 16-byte accesses");

// The best tile among those the LAST cycle did not rewrite (before the first cycle: among all), with
// its record.
struct __attribute__((aligned(16))) rest_t {
    float value;            // -1: no such tile
    int tile;
    int y, x;
    float pix[4];
};
static_assert(sizeof(rest_t) == 32, "two 16-byte accesses");

struct fused_scratch {
    fused_state st[2];
    delta_t deltas[2][1024];
    rest_t rest[2];
    owner3_t owner3[2][1024];
    // float tile_pix[tiles][4] follows
};

__device__ inline bool better_tile(float va, int ta, float vb, int tb)
{
    return va > vb || (va == vb && ta < tb);
}

// The tiles owned by thread (b, a) = (tid >> 5, tid & 31) of a 1024-thread block: (ty, tx) with
// ty % 32 == b and tx % 32 == a, visited as "slots" = 32x32-tile groups in row-major order (i.e.
// in increasing tile index).  Uniform bookkeeping, no divisions.
struct owned_tiles {
    int own, last, own_x, own_y, sup_x, tiles_x, sx, off, lim_x, lim_y, slots;

    __device__ owned_tiles(int tid, int tiles_x_, int tiles_y)
    {
        tiles_x = tiles_x_;
        sup_x = (tiles_x + 31) >> 5;
        slots = sup_x * ((tiles_y + 31) >> 5);
        last = tiles_x * tiles_y - 1;
        own_x = tid & 31;
        own_y = tid >> 5;
        own = own_y * tiles_x + own_x;
        sx = 0;
        off = 0;
        lim_x = tiles_x;
        lim_y = tiles_y;
    }

    // Tile index of the next slot (clamped into the array) and whether the slot is on the lattice
    __device__ int next(bool &valid)
    {
        const int i = min(own + off, last);
        valid = own_x < lim_x && own_y < lim_y;
        sx++;
        off += 32;
        lim_x -= 32;
        if (sx == sup_x) {
            sx = 0;
            off += 32 * tiles_x - 32 * sup_x;
            lim_x = tiles_x;
            lim_y -= 32;
        }
        return i;
    }

    // The best three owned tiles, with tile `ptile` (if >= 0) taking the value `pvalue` instead of
    // the stored one.  All of a round's loads are issued together; slots come in increasing tile
    // order, so strict comparisons keep the lowest index among equals.
    __device__ owner3_t best(const float *tile_max, int ptile, float pvalue)
    {
        owner3_t b;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            b.v[k] = -1.0f;
            b.t[k] = 0;
        }
        b.pad[0] = b.pad[1] = 0;
        for (int r = 0; r * FUSED_ROUND < slots; r++) {
            int ti[FUSED_ROUND];
            float v[FUSED_ROUND];
            bool ok[FUSED_ROUND];
#pragma unroll
            for (int k = 0; k < FUSED_ROUND; k++) {
                ti[k] = next(ok[k]);
                v[k] = tile_max[ti[k]];
            }
#pragma unroll
            for (int k = 0; k < FUSED_ROUND; k++) {
                const float val = ti[k] == ptile ? pvalue : v[k];
                if (r * FUSED_ROUND + k < slots && ok[k]) {
                    if (val > b.v[0]) {
                        b.v[2] = b.v[1];
                        b.t[2] = b.t[1];
                        b.v[1] = b.v[0];
                        b.t[1] = b.t[0];
                        b.v[0] = val;
                        b.t[0] = ti[k];
                    } else if (val > b.v[1]) {
                        b.v[2] = b.v[1];
                        b.t[2] = b.t[1];
                        b.v[1] = val;
                        b.t[1] = ti[k];
                    } else if (val > b.v[2]) {
                        b.v[2] = val;
                        b.t[2] = ti[k];
                    }
                }
            }
        }
        return b;
    }
};

__device__ inline void apply_delta(const delta_t &d, float *tile_max, int32_t *tile_pos,
                                   float *tile_pix)
{
    tile_max[d.tile] = d.value;
    tile_pos[2 * d.tile] = d.y;
    tile_pos[2 * d.tile + 1] = d.x;
#pragma unroll
    for (int p = 0; p < 4; p++)
        tile_pix[4 * d.tile + p] = d.pix[p];
}

#ifdef KIMG_CLEAN_STAMPS
#define STAMP(i) do { if (bid == 0 && tid == 0) stamps[i] = (int) wall_clock64(); } while (0)
#define KSTAMP(i) do { if (role == ROLE_KEEPER && tid == 0) stamps[i] = (int) wall_clock64(); } while (0)
#else
#define STAMP(i) do { } while (0)
#define KSTAMP(i) do { } while (0)
#endif

constexpr int ROLE_LATTICE = 0, ROLE_KEEPER = 1, ROLE_FOLDER = 2;

// The kernel is one chain of dependent steps executed once, so what counts is the latency of
// every step on the chain (global round trips ~0.8 us, LDS round trips and barriers ~0.1 us, and --
// with sixteen waves on a CU -- 0.75 us per hundred instructions of per-thread work), not
// throughput: reductions use DPP and one LDS exchange, state words travel as one 16-byte load.
// The cycle of one channel, executed by the workgroup that serves lattice block (blk_x, blk_y) of
// its PSF patch, or by one of the channel's two bookkeeping workgroups.  Two kernels call it: one
// channel per launch (cycle_fused_kernel) and several channels per launch (cycle_fused_batch_kernel).
// MASKED (one channel per launch only): candidates of the rescan are the allowed pixels, and a best
// metric of exactly 0 ends the loop whatever the threshold -- every workgroup of the launch finds
// that out for itself, like the threshold test.
template <int MODE, bool MASKED>
__device__ __attribute__((always_inline)) inline void fused_cycle(
    float *dirty, float *model, int64_t row_stride, int64_t pol_stride, int width, int height,
    int P, const float *__restrict__ psf, int64_t psf_row_stride, int64_t psf_pol_stride,
    int psf_w, int psf_h, int patch_w, int patch_h, int border, float *tile_max,
    int32_t *tile_pos, int tiles_x, int tiles_y, float loop_gain,
    fused_scratch *scratch, int parity, float *log, int blk_x, int blk_y, int role,
    const uint8_t *__restrict__ mask, int64_t mask_row_stride)
{
    __shared__ key_t s_keys[16];
    __shared__ int s_pos[2];
    __shared__ float s_pix[4];
    const fused_state *cur = &scratch->st[parity];
    fused_state *next = &scratch->st[parity ^ 1];
    const delta_t *din = scratch->deltas[parity];
    delta_t *dout = scratch->deltas[parity ^ 1];
    float *tile_pix = reinterpret_cast<float *>(scratch + 1);
    const int tid = threadIdx.x;
    const bool keeper = role == ROLE_KEEPER;
#ifdef KIMG_CLEAN_STAMPS
    const int bid = (role == ROLE_LATTICE && blk_x == 0 && blk_y == 0) ? 0 : 1;   // stamps: one lattice block
    int stamps[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
    STAMP(0);
    KSTAMP(0);

    // ---- round trip 1: state, best of the rest, the records the last cycle rewrote ----------------
    const int4 st = *reinterpret_cast<const int4 *>(cur);      // count, done, limit, threshold
    const int count = st.x, done = st.y, limit = st.z;
    const float threshold = __int_as_float(st.w);
    const int lat_x = (patch_w + TILE - 1) / TILE + 1, lat_y = (patch_h + TILE - 1) / TILE + 1;
    const bool slot = (tid & 31) < lat_x && (tid >> 5) < lat_y;
    delta_t d;
    d.tag = 0;
    if (slot)
        d = din[tid];
    const rest_t rest = scratch->rest[parity];
    if (done) {
        if (keeper && tid == 0)
            *reinterpret_cast<int4 *>(next) = make_int4(count, 1, limit, st.w);
        return;
    }
    const bool live = slot && d.tag == count + 1;
    STAMP(1);
    // The bookkeeping workgroups get the last cycle's records by OWNER through LDS (a second copy of
    // the table in memory, indexed by owner, was measured: 48 KB more to fetch cold cost more than
    // the two barriers), and their owners' best three -- 32 KB, requested only now, so that the
    // state and the deltas do not queue behind them; they arrive during the reduction below.
    __shared__ delta_t s_delta[1024];
    delta_t mine;           // the last cycle's record of the one tile of THIS owner it rewrote, if any
    mine.tag = 0;
    int4 w0 = make_int4(0, 0, 0, 0), w1 = w0;
    if (role != ROLE_LATTICE) {
        s_delta[tid].tag = 0;
        lds_barrier();
        if (live)
            s_delta[d.owner] = d;
        lds_barrier();
        mine = s_delta[tid];
        const int4 *p3 = reinterpret_cast<const int4 *>(&scratch->owner3[parity][tid]);
        w0 = p3[0];
        w1 = p3[1];
    }
    const bool pending = mine.tag == count + 1;
    if (role == ROLE_FOLDER) {
        owner3_t own3;
        own3.v[0] = __int_as_float(w0.x);
        own3.v[1] = __int_as_float(w0.y);
        own3.v[2] = __int_as_float(w0.z);
        own3.t[0] = w0.w;
        own3.t[1] = w1.x;
        own3.t[2] = w1.y;
        // Nobody waits for this workgroup within the launch.  Base arrays: the records of the last
        // cycle; owners' table: the exact best three of every owner up to the last cycle, into the
        // copy the next launch's keeper reads.
        if (live)
            apply_delta(d, tile_max, tile_pos, tile_pix);
        if (pending) {
            owned_tiles walk(tid, tiles_x, tiles_y);
            own3 = walk.best(tile_max, mine.tile, mine.value);
        }
        int4 *q3 = reinterpret_cast<int4 *>(&scratch->owner3[parity ^ 1][tid]);
        q3[0] = make_int4(__float_as_int(own3.v[0]), __float_as_int(own3.v[1]),
                          __float_as_int(own3.v[2]), own3.t[0]);
        q3[1] = make_int4(own3.t[1], own3.t[2], 0, 0);
        return;
    }
    KSTAMP(1);
    const key_t mykey = live ? make_key(d.value, d.tile) : 0;
    // (a barrier that orders LDS only: the keeper's table loads are still in flight)
    key_t best = block_max_key<true>(mykey, s_keys);
    // (the rest never contains a tile that has a delta: keys of different tiles differ)
    const key_t rest_key = rest.value >= 0.0f ? make_key(rest.value, rest.tile) : 0;
    const bool from_rest = rest_key > best;
    if (from_rest)
        best = rest_key;
    STAMP(2);
    KSTAMP(2);
    const float value = __uint_as_float((unsigned) (best >> 32));
    if (best == 0 || value < threshold || count >= limit || (MASKED && value == 0.0f)) {     // clean.py:1065-1066
        if (keeper && tid == 0)
            *reinterpret_cast<int4 *>(next) = make_int4(count, 1, limit, st.w);
        return;
    }
    if (from_rest ? tid == 0 : mykey == best) {     // exactly one thread
        s_pos[0] = from_rest ? rest.y : d.y;
        s_pos[1] = from_rest ? rest.x : d.x;
#pragma unroll
        for (int p = 0; p < 4; p++)
            s_pix[p] = from_rest ? rest.pix[p] : d.pix[p];
    }
    lds_barrier();
    const int py = s_pos[0], px = s_pos[1];
    if (value == 0.0f) {
        // a tile without any positive metric won: its record holds the (x0, y0) start position
        // of clean.py:950, whose pixel is read now, as the two-launch form does
        __syncthreads();
        if (tid < 4) {
            const bool ok = py >= 0 && py < height && px >= 0 && px < width && tid < P;
            s_pix[tid] = ok ? dirty[tid * pol_stride + (int64_t) py * row_stride + px] : 0.0f;
        }
        __syncthreads();
    }
    float scale[4];
#pragma unroll
    for (int p = 0; p < 4; p++)
        scale[p] = loop_gain * s_pix[p];                            // clean.py:1044
    STAMP(3);
    const int x0 = px - patch_w / 2, y0 = py - patch_h / 2;      // clean.py:1024-1027
    // floor division: the lattice extends into the border with negative indices
    const int bx0 = (x0 - border) >= 0 ? (x0 - border) / TILE : -((border - x0 + TILE - 1) / TILE);
    const int by0 = (y0 - border) >= 0 ? (y0 - border) / TILE : -((border - y0 + TILE - 1) / TILE);
    if (keeper) {
        owner3_t own3;
        own3.v[0] = __int_as_float(w0.x);
        own3.v[1] = __int_as_float(w0.y);
        own3.v[2] = __int_as_float(w0.z);
        own3.t[0] = w0.w;
        own3.t[1] = w1.x;
        own3.t[2] = w1.y;
        // (the model pixel is fetched now and used at the very end: its round trip must not hold
        // the first wave, and with it the reduction below, back)
        float *mp = model + (tid < P ? tid : 0) * pol_stride + (int64_t) py * row_stride + px;
        float mod = 0.0f;
        if (tid < P)
            mod = *mp;
        // The best of the rest for the NEXT launch: the best tile outside THIS cycle's lattice.  An
        // owner's candidates are its best three up to the cycle before last, with the tile the last
        // cycle rewrote (if any) at its new value, without the one tile of its own that this
        // cycle's lattice contains: whatever two of them are set aside, a tile of the three
        // remains, and no other tile of the owner is better than it.
        const int txc = bx0 + (((tid & 31) - bx0) & 31), tyc = by0 + (((tid >> 5) - by0) & 31);
        const bool in_lattice = txc < bx0 + lat_x && tyc < by0 + lat_y && txc >= 0 && txc < tiles_x
                                && tyc >= 0 && tyc < tiles_y;
        const int excluded = in_lattice ? tyc * tiles_x + txc : -1;
        const int ptile = pending ? mine.tile : -1;
        float cv = -1.0f;
        int ct = 0;
#pragma unroll
        for (int k = 0; k < 3; k++)
            if (own3.v[k] >= 0.0f && own3.t[k] != ptile && own3.t[k] != excluded
                && (cv < 0.0f || better_tile(own3.v[k], own3.t[k], cv, ct))) {
                cv = own3.v[k];
                ct = own3.t[k];
            }
        if (pending && ptile != excluded && (cv < 0.0f || better_tile(mine.value, ptile, cv, ct))) {
            cv = mine.value;
            ct = ptile;
        }
        // the candidate's record is fetched before it is known whether the candidate wins: the
        // load overlaps the block reduction instead of following it (the record of the tile the
        // last cycle rewrote is in `mine`: the folder may not have stored it yet)
        int2 cpos = make_int2(mine.y, mine.x);
        float4 cpix = make_float4(mine.pix[0], mine.pix[1], mine.pix[2], mine.pix[3]);
        if (cv >= 0.0f && ct != ptile) {
            cpos = *reinterpret_cast<const int2 *>(tile_pos + 2 * ct);
            cpix = *reinterpret_cast<const float4 *>(tile_pix + 4 * ct);
        }
        const key_t ckey = cv >= 0.0f ? make_key(cv, ct) : 0;
        KSTAMP(3);
        // (barriers that order LDS only: __syncthreads() would wait for the record loads)
        lds_barrier();                          // (s_keys is free again)
        const key_t rbest = block_max_key<true>(ckey, s_keys);
        KSTAMP(4);
        rest_t *rout = &scratch->rest[parity ^ 1];
        if (rbest == 0) {
            if (tid == 0)
                rout->value = -1.0f;
        } else if (ckey == rbest) {
            rest_t r;
            r.value = cv;
            r.tile = ct;
            r.y = cpos.x;
            r.x = cpos.y;
            r.pix[0] = cpix.x;
            r.pix[1] = cpix.y;
            r.pix[2] = cpix.z;
            r.pix[3] = cpix.w;
            *rout = r;
        }
        if (tid < P) {
            float *entry = log + (int64_t) count * (3 + P);
            if (tid == 0) {
                entry[0] = value;
                entry[1] = __int_as_float(py);
                entry[2] = __int_as_float(px);
                *reinterpret_cast<int4 *>(next) = make_int4(count + 1, 0, limit, st.w);
            }
            entry[3 + tid] = scale[tid];
            *mp = mod + scale[tid];                                 // clean.py:1047
        }
#ifdef KIMG_CLEAN_STAMPS
        if (cpix.x == 12345.678f)
            stamps[7] = 1;                      // (forces the record load to complete before the stamp)
        KSTAMP(5);
        if (tid == 0)
            for (int i = 0; i < 6; i++)
                next->pad[6 + i] = stamps[i];
#endif
        return;
    }

    // ---- round trip 2: this block's pixels -----------------------------------------------
    const int tx = bx0 + blk_x, ty = by0 + blk_y;
    const int ox = tx * TILE + border, oy = ty * TILE + border;
    const int psf_dx = psf_w / 2 - px, psf_dy = psf_h / 2 - py;
    const bool is_tile = tx >= 0 && tx < tiles_x && ty >= 0 && ty < tiles_y;
    const int x = ox + (tid & 31), y = oy + (tid >> 5);
    const bool inside = x >= 0 && x < width && y >= 0 && y < height;
    const int64_t ia = (int64_t) y * row_stride + x;
    const bool in_patch = inside && x >= x0 && x < x0 + patch_w && y >= y0 && y < y0 + patch_h;
    bool in_tile = inside && is_tile && x < width - border && y < height - border;
    float dv[4] = {0.0f, 0.0f, 0.0f, 0.0f}, pv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    // (the mask byte travels with the pixel loads: no round trip of its own)
    uint8_t allowed = 1;
    if (MASKED && in_tile)
        allowed = mask[(int64_t) y * mask_row_stride + x];
    if (inside)
        for (int p = 0; p < P; p++)
            dv[p] = dirty[p * pol_stride + ia];
    if (in_patch)
        for (int p = 0; p < P; p++)
            pv[p] = psf[p * psf_pol_stride + (int64_t) (y + psf_dy) * psf_row_stride + (x + psf_dx)];
    float metric = 0.0f;
#ifdef KIMG_CLEAN_STAMPS
    if (dv[0] + pv[0] == 12345.678f)
        stamps[7] = 1;
    STAMP(4);
#endif
    for (int p = 0; p < P; p++) {
        if (in_patch) {
            const float tp = scale[p] * pv[p];
            dv[p] -= tp;
            dirty[p * pol_stride + ia] = dv[p];
        }
        if (MODE == KIMG_CLEAN_I) {
            if (p == 0)
                metric = fabsf(dv[0]);
        } else {
            metric += dv[p] * dv[p];
        }
    }
    if (!is_tile)
        return;
    if (MASKED)
        in_tile = in_tile && allowed;
    // first strict maximum in row-major order; only positive metrics count (clean.py:953-958)
    const key_t tb = block_max_key((in_tile && metric > 0.0f) ? make_key(metric, tid) : 0, s_keys);
    const int widx = ~(int) (unsigned) tb;
#ifdef KIMG_CLEAN_STAMPS
    STAMP(5);
    if (bid == 0 && tid == 0)
        for (int i = 0; i < 6; i++)
            next->pad[i] = stamps[i];
#endif
    if (tb == 0 ? tid == 0 : tid == widx) {
        delta_t o;
        o.tag = count + 2;
        o.tile = ty * tiles_x + tx;
        if (tb == 0) {
            // no positive metric: value 0 and the (x0, y0) initial position of clean.py:950; the
            // pixel there is read when (if ever) this tile wins, see above
            o.value = 0.0f;
            o.y = ox;
            o.x = oy;
#pragma unroll
            for (int p = 0; p < 4; p++)
                o.pix[p] = 0.0f;
        } else {
            o.value = metric;
            o.y = y;
            o.x = x;
#pragma unroll
            for (int p = 0; p < 4; p++)
                o.pix[p] = dv[p];
        }
        o.owner = (ty & 31) * 32 + (tx & 31);
        o.pad[0] = o.pad[1] = 0;
        dout[blk_y * 32 + blk_x] = o;
    }
}

template <int MODE>
__global__ __launch_bounds__(1024) void cycle_fused_kernel(
    float *dirty, float *model, int64_t row_stride, int64_t pol_stride, int width, int height,
    int P, const float *__restrict__ psf, int64_t psf_row_stride, int64_t psf_pol_stride,
    int psf_w, int psf_h, int patch_w, int patch_h, int border, float *tile_max,
    int32_t *tile_pos, int tiles_x, int tiles_y, float loop_gain,
    fused_scratch *scratch, int parity, float *log)
{
    // The FIRST row of the grid (dispatched first) holds the two bookkeeping workgroups instead of
    // lattice blocks (its other members have nothing to do; a lattice is at least two blocks wide).
    int role = ROLE_LATTICE;
    if (blockIdx.y == 0) {
        if (blockIdx.x > 1)
            return;
        role = blockIdx.x == 0 ? ROLE_KEEPER : ROLE_FOLDER;
    }
    fused_cycle<MODE, false>(dirty, model, row_stride, pol_stride, width, height, P, psf,
                             psf_row_stride, psf_pol_stride, psf_w, psf_h, patch_w, patch_h, border,
                             tile_max, tile_pos, tiles_x, tiles_y, loop_gain, scratch, parity, log,
                             (int) blockIdx.x, (int) blockIdx.y - 1, role, nullptr, 0);
}

template <int MODE>
__global__ __launch_bounds__(1024) void cycle_fused_masked_kernel(
    float *dirty, float *model, int64_t row_stride, int64_t pol_stride, int width, int height,
    int P, const float *__restrict__ psf, int64_t psf_row_stride, int64_t psf_pol_stride,
    int psf_w, int psf_h, int patch_w, int patch_h, int border, float *tile_max,
    int32_t *tile_pos, int tiles_x, int tiles_y, float loop_gain,
    fused_scratch *scratch, int parity, float *log, const uint8_t *__restrict__ mask,
    int64_t mask_row_stride)
{
    // (the grid of cycle_fused_kernel)
    int role = ROLE_LATTICE;
    if (blockIdx.y == 0) {
        if (blockIdx.x > 1)
            return;
        role = blockIdx.x == 0 ? ROLE_KEEPER : ROLE_FOLDER;
    }
    fused_cycle<MODE, true>(dirty, model, row_stride, pol_stride, width, height, P, psf,
                            psf_row_stride, psf_pol_stride, psf_w, psf_h, patch_w, patch_h, border,
                            tile_max, tile_pos, tiles_x, tiles_y, loop_gain, scratch, parity, log,
                            (int) blockIdx.x, (int) blockIdx.y - 1, role, mask, mask_row_stride);
}

// ---- several channels per launch -------------------------------------------------------------
// A minor cycle is a latency chain (kernel boundary 2.1 us + ~3 us of dependent work) that
// occupies 32 of the 256 CUs.  Channels of a band are independent and have
// images of the same shape, so cycle i of up to KIMG_CLEAN_BATCH_MAX channels runs as ONE launch:
// blockIdx.z is the channel, whose pointers, patch size and (through its own state words)
// threshold, cycle limit and stop flag are its own; a finished channel's workgroups return after
// their first load.  The boundary and the cold load are paid once for all of them.  The table of
// channels travels in the kernel arguments (scalar loads with a uniform index: no extra round trip).
struct batch_channel {
    float *dirty, *model;
    const float *psf;
    float *tile_max;
    int32_t *tile_pos;
    fused_scratch *scratch;
    float *log;
    int patch_w, patch_h;
};

struct batch_table {
    batch_channel ch[KIMG_CLEAN_BATCH_MAX];
};

template <int MODE>
__global__ __launch_bounds__(1024) void cycle_fused_batch_kernel(
    batch_table tab, int64_t row_stride, int64_t pol_stride, int width, int height, int P,
    int64_t psf_row_stride, int64_t psf_pol_stride, int psf_w, int psf_h, int border, int tiles_x,
    int tiles_y, float loop_gain, int parity)
{
    // grid = (largest number of lattice blocks of any channel + 2, 1, channels): blocks 0 and 1 of a
    // channel keep its books, blocks 2 .. bx * by + 1 serve its lattice row by row; no workgroup is
    // launched only to find that it has nothing to do unless the channels' patches differ in size
    // (8 channels with the 6 x 5 lattice blocks of a 133 x 111 patch are 256 workgroups: one per CU)
    const batch_channel &ch = tab.ch[blockIdx.z];
    const int bx = (ch.patch_w + TILE - 1) / TILE + 1, by = (ch.patch_h + TILE - 1) / TILE + 1;
    const int role = blockIdx.x == 0 ? ROLE_KEEPER : blockIdx.x == 1 ? ROLE_FOLDER : ROLE_LATTICE;
    int blk_x = (int) blockIdx.x - 2, blk_y = 0;
    if (blk_x >= bx * by)
        return;
    while (blk_x >= bx) {           // (uniform; at most 31 rounds, typically < 6)
        blk_x -= bx;
        blk_y++;
    }
    fused_cycle<MODE, false>(ch.dirty, ch.model, row_stride, pol_stride, width, height, P, ch.psf,
                             psf_row_stride, psf_pol_stride, psf_w, psf_h, ch.patch_w, ch.patch_h,
                             border, ch.tile_max, ch.tile_pos, tiles_x, tiles_y, loop_gain,
                             ch.scratch, parity, ch.log, blk_x, blk_y, role, nullptr, 0);
}

// Pixel values at every tile's peak position (the part of a tile record the tile scan of
// kimg_update_tiles does not produce); once per kimg_clean_cycles call.
__global__ __launch_bounds__(256) void tile_pix_kernel(
    const float *__restrict__ dirty, int64_t row_stride, int64_t pol_stride, int width,
    int height, int P, const int32_t *__restrict__ tile_pos, int num_tiles,
    fused_scratch *scratch)
{
    float *tile_pix = reinterpret_cast<float *>(scratch + 1);
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= num_tiles)
        return;
    const int y = tile_pos[2 * t], x = tile_pos[2 * t + 1];
    const bool ok = y >= 0 && y < height && x >= 0 && x < width;
    for (int p = 0; p < 4; p++)
        tile_pix[4 * t + p] = (ok && p < P) ? dirty[p * pol_stride + (int64_t) y * row_stride + x] : 0.0f;
}

// Every owner's best three tiles (into the copy of the table the first launch's keeper reads) and
// the best tile of all with its record, the first launch's `rest` (see fused_cycle); once per
// kimg_clean_cycles call, after tile_pix_kernel.
__global__ __launch_bounds__(1024) void owner_best_kernel(const float *__restrict__ tile_max,
                                                          const int32_t *__restrict__ tile_pos,
                                                          int tiles_x, int tiles_y,
                                                          fused_scratch *scratch)
{
    __shared__ key_t s_keys[16];
    const float *tile_pix = reinterpret_cast<const float *>(scratch + 1);
    owned_tiles walk(threadIdx.x, tiles_x, tiles_y);
    const owner3_t b = walk.best(tile_max, -1, 0.0f);
    scratch->owner3[0][threadIdx.x] = b;
    const key_t key = b.v[0] >= 0.0f ? make_key(b.v[0], b.t[0]) : 0;
    const key_t best = block_max_key(key, s_keys);
    rest_t *rout = &scratch->rest[0];
    if (best == 0) {
        if (threadIdx.x == 0)
            rout->value = -1.0f;
    } else if (key == best) {
        rest_t r;
        r.value = b.v[0];
        r.tile = b.t[0];
        r.y = tile_pos[2 * b.t[0]];
        r.x = tile_pos[2 * b.t[0] + 1];
#pragma unroll
        for (int p = 0; p < 4; p++)
            r.pix[p] = tile_pix[4 * b.t[0] + p];
        *rout = r;
    }
}

// Fold the deltas of the last cycle into the base tile arrays (the state left by an even number
// of cycle launches is st[0], its pending deltas are deltas[0]).
__global__ __launch_bounds__(1024) void apply_deltas_kernel(fused_scratch *scratch, float *tile_max,
                                                            int32_t *tile_pos)
{
    float *tile_pix = reinterpret_cast<float *>(scratch + 1);
    const delta_t d = scratch->deltas[0][threadIdx.x];
    if (d.tag == scratch->st[0].count + 1)
        apply_delta(d, tile_max, tile_pos, tile_pix);
}

// ---- PSF patch bound ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void psf_patch_kernel(
    const float *__restrict__ psf, int64_t row_stride, int64_t pol_stride, int P,
    int min_x, int min_y, int max_x, int max_y, int mid_x, int mid_y, float threshold,
    int32_t *__restrict__ bound)
{
    int dx = 0, dy = 0;
    for (int y = min_y + blockIdx.y; y <= max_y; y += gridDim.y)
        for (int x = min_x + blockIdx.x * blockDim.x + threadIdx.x; x <= max_x;
             x += gridDim.x * blockDim.x) {
            bool over = false;
            for (int p = 0; p < P; p++)
                over |= fabsf(psf[p * pol_stride + (int64_t) y * row_stride + x]) >= threshold;
            if (over) {
                dx = max(dx, abs(x - mid_x));
                dy = max(dy, abs(y - mid_y));
            }
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        dx = max(dx, __shfl_xor(dx, off, WAVE));
        dy = max(dy, __shfl_xor(dy, off, WAVE));
    }
    if ((threadIdx.x & 63) == 0 && (dx | dy)) {
        atomicMax(&bound[0], dx);
        atomicMax(&bound[1], dy);
    }
}

// ---- noise estimate: radix select on the bit pattern of |x| ------------------------------
__global__ __launch_bounds__(256) void abs_histogram_kernel(
    const float *__restrict__ image, int64_t row_stride, int64_t pol_stride, int width,
    int height, int P, int border, int pass, uint32_t prefix, uint32_t *__restrict__ hist)
{
    __shared__ uint32_t local[256];
    local[threadIdx.x] = 0;
    __syncthreads();
    const int shift = 8 * pass;
    // Run-length accumulation: in the first pass (sign-less exponent byte) nearly every pixel
    // of a noise-like image falls into the same two or three bins, and one LDS atomic per
    // pixel would serialise the whole wave on them.
    uint32_t run_bin = 0, run = 0;
    // four rows per round, their loads issued together (the loop is otherwise one dependent
    // memory round trip per pixel row)
    constexpr int ROWS = 4;
    const int x = border + blockIdx.x * blockDim.x + threadIdx.x;
    const bool x_ok = x < width - border;
    for (int p = 0; p < P; p++)
        for (int y0 = border + blockIdx.y; y0 < height - border; y0 += gridDim.y * ROWS) {
            uint32_t keys[ROWS];
            bool ok[ROWS];
#pragma unroll
            for (int r = 0; r < ROWS; r++) {
                const int y = y0 + r * gridDim.y;
                ok[r] = x_ok && y < height - border;
                keys[r] = ok[r] ? __float_as_uint(image[p * pol_stride + (int64_t) y * row_stride + x])
                                      & 0x7fffffffu : 0u;
            }
#pragma unroll
            for (int r = 0; r < ROWS; r++) {
                const uint32_t key = keys[r];
                if (ok[r] && (pass == 3 || (key >> (shift + 8)) == prefix)) {
                    const uint32_t bin = (key >> shift) & 255u;
                    if (bin != run_bin) {
                        if (run)
                            atomicAdd(&local[run_bin], run);
                        run_bin = bin;
                        run = 0;
                    }
                    run++;
                }
            }
        }
    if (run)
        atomicAdd(&local[run_bin], run);
    __syncthreads();
    if (local[threadIdx.x])
        atomicAdd(&hist[threadIdx.x], local[threadIdx.x]);
}

__global__ __launch_bounds__(256) void abs_count_le_kernel(
    const float *__restrict__ image, int64_t row_stride, int64_t pol_stride, int width,
    int height, int P, int border, uint32_t value_bits, uint32_t *__restrict__ out)
{
    uint32_t count = 0, next = 0xffffffffu;
    constexpr int ROWS = 8;
    const int x = border + blockIdx.x * blockDim.x + threadIdx.x;
    const bool x_ok = x < width - border;
    for (int p = 0; p < P; p++)
        for (int y0 = border + blockIdx.y; y0 < height - border; y0 += gridDim.y * ROWS) {
            uint32_t keys[ROWS];
            bool ok[ROWS];
#pragma unroll
            for (int r = 0; r < ROWS; r++) {
                const int y = y0 + r * gridDim.y;
                ok[r] = x_ok && y < height - border;
                keys[r] = ok[r] ? __float_as_uint(image[p * pol_stride + (int64_t) y * row_stride + x])
                                      & 0x7fffffffu : 0u;
            }
#pragma unroll
            for (int r = 0; r < ROWS; r++)
                if (ok[r]) {
                    if (keys[r] <= value_bits)
                        count++;
                    else
                        next = min(next, keys[r]);
                }
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        count += __shfl_xor(count, off, WAVE);
        next = min(next, (uint32_t) __shfl_xor((int) next, off, WAVE));
    }
    // one pair of atomics per workgroup (same-address atomics from thousands of waves serialise)
    __shared__ uint32_t s_count[4], s_next[4];
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_count[wv] = count;
        s_next[wv] = next;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int) (blockDim.x >> 6); w++) {
            count += s_count[w];
            next = min(next, s_next[w]);
        }
        if (count)
            atomicAdd(&out[0], count);
        if (next != 0xffffffffu)
            atomicMin(&out[1], next);
    }
}

dim3 region_grid(int width, int height, int max_blocks = 2048)
{
    int bx = kimg_divup(width, 256);
    if (bx < 1) bx = 1;
    int by = height < max_blocks / bx ? height : max_blocks / bx;
    return dim3(bx, by > 0 ? by : 1);
}

} // namespace

// kimg_update_tiles and kimg_update_tiles_masked (mask null: unmasked)
static int update_tiles(const float *dirty, int64_t row_stride, int64_t pol_stride,
                        int width, int height, int num_polarizations, int border,
                        int mode, float *tile_max, int32_t *tile_pos, int tiles_x,
                        int tiles_y, int tile_x0, int tile_y0, int tile_x1, int tile_y1,
                        const uint8_t *mask, int64_t mask_row_stride, void *stream)
{
    KIMG_CHECK_ARG(dirty && tile_max && tile_pos && width > 0 && height > 0 && row_stride >= width);
    KIMG_CHECK_ARG(num_polarizations >= 1 && num_polarizations <= 4 && border >= 0);
    KIMG_CHECK_ARG(tile_x0 >= 0 && tile_y0 >= 0 && tile_x1 <= tiles_x && tile_y1 <= tiles_y);
    if (tile_x0 >= tile_x1 || tile_y0 >= tile_y1)
        return 0;                                           // clean.py:462
    KIMG_CHECK_ARG(mask == nullptr || mask_row_stride >= width);
    dim3 g(tile_x1 - tile_x0, tile_y1 - tile_y0);
    hipStream_t s = (hipStream_t) stream;
    const bool known = kimg_for_clean_mode(mode, [&](auto m) {
        constexpr int MODE = decltype(m)::value;
        if (mask != nullptr)
            update_tiles_masked_kernel<MODE><<<g, 256, 0, s>>>(
                dirty, row_stride, pol_stride, width, height, num_polarizations, border, tile_max,
                tile_pos, tiles_x, tile_x0, tile_y0, mask, mask_row_stride);
        else
            update_tiles_kernel<MODE><<<g, 256, 0, s>>>(
                dirty, row_stride, pol_stride, width, height, num_polarizations, border, tile_max,
                tile_pos, tiles_x, tile_x0, tile_y0); });
    return known ? kimg_launch_status() : KIMG_EINVAL;
}

extern "C" int kimg_update_tiles(const float *dirty, int64_t row_stride, int64_t pol_stride,
                                 int width, int height, int num_polarizations, int border,
                                 int mode, float *tile_max, int32_t *tile_pos, int tiles_x,
                                 int tiles_y, int tile_x0, int tile_y0, int tile_x1, int tile_y1,
                                 void *stream)
{
    return update_tiles(dirty, row_stride, pol_stride, width, height, num_polarizations, border, mode,
                        tile_max, tile_pos, tiles_x, tiles_y, tile_x0, tile_y0, tile_x1, tile_y1,
                        nullptr, 0, stream);
}

extern "C" int kimg_update_tiles_masked(const float *dirty, int64_t row_stride, int64_t pol_stride,
                                        int width, int height, int num_polarizations, int border,
                                        int mode, float *tile_max, int32_t *tile_pos, int tiles_x,
                                        int tiles_y, int tile_x0, int tile_y0, int tile_x1,
                                        int tile_y1, void *stream, const uint8_t *mask,
                                        int64_t mask_row_stride)
{
    return update_tiles(dirty, row_stride, pol_stride, width, height, num_polarizations, border, mode,
                        tile_max, tile_pos, tiles_x, tiles_y, tile_x0, tile_y0, tile_x1, tile_y1,
                        mask, mask_row_stride, stream);
}

// kimg_find_peak and kimg_find_peak_masked (mask null: unmasked)
static int find_peak_call(const float *dirty, int64_t row_stride, int64_t pol_stride,
                          int num_polarizations, const float *tile_max,
                          const int32_t *tile_pos, int tiles_x, int tiles_y,
                          float *peak_value, int32_t *peak_pos, float *peak_pixel,
                          const uint8_t *mask, void *stream)
{
    KIMG_CHECK_ARG(dirty && tile_max && tile_pos && peak_value && peak_pos && peak_pixel);
    KIMG_CHECK_ARG(tiles_x > 0 && tiles_y > 0 && num_polarizations >= 1);
    if (mask != nullptr)
        find_peak_masked_kernel<<<1, 1024, 0, (hipStream_t) stream>>>(
            dirty, row_stride, pol_stride, num_polarizations, tile_max, tile_pos, tiles_x * tiles_y,
            peak_value, peak_pos, peak_pixel);
    else
        find_peak_kernel<<<1, 1024, 0, (hipStream_t) stream>>>(
            dirty, row_stride, pol_stride, num_polarizations, tile_max, tile_pos, tiles_x * tiles_y,
            peak_value, peak_pos, peak_pixel);
    return kimg_launch_status();
}

extern "C" int kimg_find_peak(const float *dirty, int64_t row_stride, int64_t pol_stride,
                              int num_polarizations, const float *tile_max,
                              const int32_t *tile_pos, int tiles_x, int tiles_y,
                              float *peak_value, int32_t *peak_pos, float *peak_pixel,
                              void *stream)
{
    return find_peak_call(dirty, row_stride, pol_stride, num_polarizations, tile_max, tile_pos, tiles_x,
                          tiles_y, peak_value, peak_pos, peak_pixel, nullptr, stream);
}

extern "C" int kimg_find_peak_masked(const float *dirty, int64_t row_stride, int64_t pol_stride,
                                     int num_polarizations, const float *tile_max,
                                     const int32_t *tile_pos, int tiles_x, int tiles_y,
                                     float *peak_value, int32_t *peak_pos, float *peak_pixel,
                                     void *stream, const uint8_t *mask, int64_t mask_row_stride)
{
    (void) mask_row_stride;     // (the peak step needs to know THAT a mask is bound, not its bytes)
    return find_peak_call(dirty, row_stride, pol_stride, num_polarizations, tile_max, tile_pos, tiles_x,
                          tiles_y, peak_value, peak_pos, peak_pixel, mask, stream);
}

extern "C" int kimg_subtract_psf(float *dirty, float *model, int64_t row_stride,
                                 int64_t pol_stride, int width, int height, int num_polarizations,
                                 const float *psf, int64_t psf_row_stride, int64_t psf_pol_stride,
                                 int psf_width, int psf_height, int patch_width, int patch_height,
                                 const float *peak_pixel, int pos_x, int pos_y, float loop_gain,
                                 void *stream)
{
    KIMG_CHECK_ARG(dirty && model && psf && peak_pixel);
    KIMG_CHECK_ARG(num_polarizations >= 1 && num_polarizations <= 4);
    KIMG_CHECK_ARG(patch_width > 0 && patch_height > 0 && patch_width <= psf_width
                   && patch_height <= psf_height);
    KIMG_CHECK_ARG(pos_x >= 0 && pos_x < width && pos_y >= 0 && pos_y < height);
    KIMG_CHECK_ARG(row_stride >= width && psf_row_stride >= psf_width);
    const int psf_x0 = psf_width / 2 - patch_width / 2;     // clean.py:699-700
    const int psf_y0 = psf_height / 2 - patch_height / 2;
    dim3 g(kimg_divup(patch_width, 64), kimg_divup(patch_height, 4));
    subtract_psf_kernel<<<g, 256, 0, (hipStream_t) stream>>>(
        dirty, model, row_stride, pol_stride, width, height, num_polarizations, psf,
        psf_row_stride, psf_pol_stride, psf_x0, psf_y0, patch_width, patch_height, peak_pixel,
        pos_x, pos_y, pos_x - patch_width / 2, pos_y - patch_height / 2, loop_gain);
    return kimg_launch_status();
}

extern "C" size_t kimg_clean_state_bytes(int num_polarizations, int tiles_x, int tiles_y)
{
    (void) num_polarizations;
    static_assert(sizeof(fused_scratch) >= sizeof(clean_state), "the two forms share the scratch");
    if (tiles_x <= 0 || tiles_y <= 0)
        return 0;
    // the one-launch form's scratch with its tile_pix[tiles][4]
    const size_t n = sizeof(fused_scratch) + (size_t) tiles_x * tiles_y * 4 * sizeof(float);
    const size_t m = kimg_clean_multi_state_bytes(tiles_x, tiles_y);
    return n > m ? n : m;
}

namespace {

__global__ void init_state_kernel(clean_state *state, int limit, float threshold)
{
    state->limit = limit;
    state->threshold = threshold;
}

struct cycle_args {
    float *dirty, *model;
    int64_t row_stride, pol_stride;
    int width, height, P;
    const float *psf;
    int64_t psf_row_stride, psf_pol_stride;
    int psf_width, psf_height, patch_width, patch_height, border, mode;
    float loop_gain;
    float *tile_max;
    int32_t *tile_pos;
    int tiles_x, tiles_y;
    clean_state *state;
    float *log;
    const uint8_t *mask;    // null: unmasked (never set for a batch)
    int64_t mask_row_stride;
    int fused;              // one launch per cycle (state is then a fused_scratch)
    int batch;              // > 0: that many channels per launch, described by `tab` (the fields
                            // dirty .. log, patch_width / patch_height above are then unused)
    int batch_blocks;       // largest number of lattice blocks over the batch's channels
    batch_table tab;
};

// One minor cycle: one launch for a batch or the one-launch form, else two dependent launches (peak +
// threshold test, then subtract + tile update).  (Callers have checked the mode.)
int enqueue_cycle(const cycle_args &a, hipStream_t s, int index)
{
    kimg_for_clean_mode(a.mode, [&](auto m) {
        constexpr int MODE = decltype(m)::value;
        if (a.batch > 0) {
            const dim3 gb(a.batch_blocks + 2, 1, a.batch);          // + the two bookkeeping workgroups
            cycle_fused_batch_kernel<MODE><<<gb, 1024, 0, s>>>(
                a.tab, a.row_stride, a.pol_stride, a.width, a.height, a.P, a.psf_row_stride,
                a.psf_pol_stride, a.psf_width, a.psf_height, a.border, a.tiles_x, a.tiles_y,
                a.loop_gain, index & 1);
            return;
        }
        dim3 g(kimg_divup(a.patch_width, TILE) + 1, kimg_divup(a.patch_height, TILE) + 1);
        if (a.fused) {
            fused_scratch *fs = reinterpret_cast<fused_scratch *>(a.state);
            g.y += 1;               // the bookkeeping workgroup's row
            if (a.mask != nullptr)
                cycle_fused_masked_kernel<MODE><<<g, 1024, 0, s>>>(
                    a.dirty, a.model, a.row_stride, a.pol_stride, a.width, a.height, a.P, a.psf,
                    a.psf_row_stride, a.psf_pol_stride, a.psf_width, a.psf_height, a.patch_width,
                    a.patch_height, a.border, a.tile_max, a.tile_pos, a.tiles_x, a.tiles_y,
                    a.loop_gain, fs, index & 1, a.log, a.mask, a.mask_row_stride);
            else
                cycle_fused_kernel<MODE><<<g, 1024, 0, s>>>(
                    a.dirty, a.model, a.row_stride, a.pol_stride, a.width, a.height, a.P, a.psf,
                    a.psf_row_stride, a.psf_pol_stride, a.psf_width, a.psf_height, a.patch_width,
                    a.patch_height, a.border, a.tile_max, a.tile_pos, a.tiles_x, a.tiles_y,
                    a.loop_gain, fs, index & 1, a.log);
            return;
        }
        const int num_tiles = a.tiles_x * a.tiles_y;
        if (a.mask != nullptr) {
            cycle_find_peak_masked_kernel<<<1, 1024, 0, s>>>(
                a.dirty, a.model, a.row_stride, a.pol_stride, a.P, a.tile_max, a.tile_pos, num_tiles,
                a.loop_gain, a.state, a.log);
            cycle_subtract_update_masked_kernel<MODE><<<g, 256, 0, s>>>(
                a.dirty, a.row_stride, a.pol_stride, a.width, a.height, a.P, a.psf, a.psf_row_stride,
                a.psf_pol_stride, a.psf_width, a.psf_height, a.patch_width, a.patch_height, a.border,
                a.tile_max, a.tile_pos, a.tiles_x, a.tiles_y, a.state, a.mask, a.mask_row_stride);
        } else {
            cycle_find_peak_kernel<MODE><<<1, 1024, 0, s>>>(
                a.dirty, a.model, a.row_stride, a.pol_stride, a.P, a.tile_max, a.tile_pos, num_tiles,
                a.loop_gain, a.state, a.log);
            cycle_subtract_update_kernel<MODE><<<g, 256, 0, s>>>(
                a.dirty, a.row_stride, a.pol_stride, a.width, a.height, a.P, a.psf, a.psf_row_stride,
                a.psf_pol_stride, a.psf_width, a.psf_height, a.patch_width, a.patch_height, a.border,
                a.tile_max, a.tile_pos, a.tiles_x, a.tiles_y, a.state);
        } });
    return kimg_launch_status();
}

// hipGraph of GRAPH_CYCLES minor cycles, cached per argument set (kimg_graph_cache.h).  The
// device-side `limit` makes surplus cycles of the last replay no-ops.
#ifndef KIMG_GRAPH_CYCLES
#define KIMG_GRAPH_CYCLES 64
#endif
constexpr int GRAPH_CYCLES = KIMG_GRAPH_CYCLES;
// the one-launch form alternates two state / delta buffers by launch parity and must leave the
// final state in st[0]: a replay has to be an even number of launches
static_assert(GRAPH_CYCLES >= 2 && GRAPH_CYCLES % 2 == 0, "KIMG_GRAPH_CYCLES must be even");
// 32 argument sets (channels in flight x patch sizes)
kimg_graph_cache<cycle_args, 32> graph_cache;

// `max_cycles` minor cycles on `s`: replays of the cached graph when the call is long enough to be
// worth one (and the cache has one to give), plain launches otherwise.
int run_cycles(const cycle_args &a, int max_cycles, hipStream_t s)
{
    int done = 0;
    if (max_cycles >= GRAPH_CYCLES / 2) {
        auto *entry = graph_cache.acquire(a, [&](hipStream_t cs) {
            int rc = 0;
            for (int i = 0; i < GRAPH_CYCLES && rc == 0; i++)
                rc = enqueue_cycle(a, cs, i);
            return rc; });
        if (entry) {
            hipError_t e = hipSuccess;
            for (; done < max_cycles && e == hipSuccess; done += GRAPH_CYCLES)
                e = hipGraphLaunch(entry->exec, s);
            graph_cache.release(entry, s);
            if (e != hipSuccess)
                return -(int) e;
            done = max_cycles;
        }
    }
    // (an even number of launches, so that the one-launch form leaves its state in st[0]; the
    // device-side limit makes the surplus one a no-op)
    for (int i = 0; done < max_cycles || (i & 1); done++, i++) {
        const int rc = enqueue_cycle(a, s, i);
        if (rc)
            return rc;
    }
    return 0;
}

// The fields of `a` that a single channel's call and a batch share.  (The memset comes first: padding
// bytes take part in the cache key comparison.)
void fill_shared(cycle_args &a, int64_t row_stride, int64_t pol_stride, int width, int height, int P,
                 int64_t psf_row_stride, int64_t psf_pol_stride, int psf_width, int psf_height,
                 int border, int mode, float loop_gain, int tiles_x, int tiles_y, bool fused)
{
    memset(&a, 0, sizeof(a));
    a.row_stride = row_stride; a.pol_stride = pol_stride; a.width = width; a.height = height;
    a.P = P; a.psf_row_stride = psf_row_stride; a.psf_pol_stride = psf_pol_stride;
    a.psf_width = psf_width; a.psf_height = psf_height; a.border = border; a.mode = mode;
    a.loop_gain = loop_gain; a.tiles_x = tiles_x; a.tiles_y = tiles_y; a.fused = fused;
}

// One launch per cycle: when the patch touches few lattice blocks (every workgroup then repeats the
// global peak search) ...
bool patch_fits_one_launch(int patch_width, int patch_height)
{
    const int bx = kimg_divup(patch_width, TILE) + 1, by = kimg_divup(patch_height, TILE) + 1;
    return bx * (by + 1) <= FUSED_MAX_BLOCKS && bx <= 32 && by <= 32;
}

// ... and the tiles' owners (one per 32 x 32 tiles) fit the scratch
bool tiles_fit_one_launch(int tiles_x, int tiles_y)
{
    return kimg_divup(tiles_x, 32) * kimg_divup(tiles_y, 32) <= FUSED_MAX_SLOTS;
}

// One channel's scratch at the start of a call: the loop's limit and threshold and, for the one-launch
// form, the peak pixels of every tile ...
int begin_state(const cycle_args &a, void *state, int max_cycles, float threshold, const float *dirty,
                const int32_t *tile_pos, hipStream_t s)
{
    KIMG_HIP(hipMemsetAsync(state, 0, sizeof(fused_scratch), s));
    init_state_kernel<<<1, 1, 0, s>>>(static_cast<clean_state *>(state), max_cycles, threshold);
    if (a.fused)
        tile_pix_kernel<<<kimg_divup(a.tiles_x * a.tiles_y, 256), 256, 0, s>>>(
            dirty, a.row_stride, a.pol_stride, a.width, a.height, a.P, tile_pos, a.tiles_x * a.tiles_y,
            static_cast<fused_scratch *>(state));
    return 0;
}

// ... then every owner's best two tiles, before the first cycle of the one-launch form ...
void begin_owners(const cycle_args &a, void *state, float *tile_max, int32_t *tile_pos, hipStream_t s)
{
    owner_best_kernel<<<1, 1024, 0, s>>>(tile_max, tile_pos, a.tiles_x, a.tiles_y,
                                         static_cast<fused_scratch *>(state));
}

// ... and after its last one, the tile records brought up to date
void end_state(void *state, float *tile_max, int32_t *tile_pos, hipStream_t s)
{
    apply_deltas_kernel<<<1, 1024, 0, s>>>(static_cast<fused_scratch *>(state), tile_max, tile_pos);
}

} // namespace

// The minor cycles of one major cycle in one call (frontend.py:560-585): the first cycle runs without
// a threshold, the threshold of the rest follows from its peak on the device.  Only where the
// multi-component form runs (KIMG_EUNSUPPORTED otherwise: the caller takes kimg_clean_cycles then).
extern "C" int kimg_clean_major_cycles(float *dirty, float *model, int64_t row_stride,
                                       int64_t pol_stride, int width, int height, int num_polarizations,
                                       const float *psf, int64_t psf_row_stride, int64_t psf_pol_stride,
                                       int psf_width, int psf_height, int patch_width, int patch_height,
                                       int border, int mode, float loop_gain, double noise_threshold,
                                       double left_for_next, float *tile_max, int32_t *tile_pos,
                                       int tiles_x, int tiles_y, int max_cycles, int form, void *state,
                                       float *log, void *stream, int *cycles_done, float *first_peak)
{
    KIMG_CHECK_ARG(dirty && model && psf && tile_max && tile_pos && state && log);
    KIMG_CHECK_ARG(num_polarizations >= 1 && num_polarizations <= 4 && max_cycles >= 1);
    KIMG_CHECK_ARG(patch_width > 0 && patch_height > 0 && patch_width <= psf_width
                   && patch_height <= psf_height && tiles_x > 0 && tiles_y > 0);
    KIMG_CHECK_ARG(mode == KIMG_CLEAN_I || mode == KIMG_CLEAN_SUMSQ);
    KIMG_CHECK_ARG(row_stride >= width && psf_row_stride >= psf_width);
    KIMG_CHECK_ARG(noise_threshold == noise_threshold && left_for_next == left_for_next);      // (not NaN)
    const int kind = form & 0xff;
    KIMG_CHECK_ARG(kind == KIMG_CLEAN_FORM_AUTO || kind == KIMG_CLEAN_FORM_MULTI);
    if (kimg_clean_multi_components(patch_width, patch_height, tiles_x, tiles_y) < (kind == KIMG_CLEAN_FORM_MULTI ? 1 : 2))
        return KIMG_EUNSUPPORTED;
    return kimg_clean_multi_run(dirty, model, row_stride, pol_stride, width, height, num_polarizations, psf,
                                psf_row_stride, psf_pol_stride, psf_width, psf_height, patch_width,
                                patch_height, border, mode, loop_gain, 0.0f, tile_max, tile_pos, tiles_x,
                                tiles_y, max_cycles, (form >> 8) & 0xff, (form >> 16) & 0x1f, true,
                                noise_threshold, left_for_next, state, log, (hipStream_t) stream, cycles_done,
                                first_peak);
}

// kimg_clean_cycles and kimg_clean_cycles_masked (mask null: unmasked)
static int clean_cycles(float *dirty, float *model, int64_t row_stride,
                        int64_t pol_stride, int width, int height, int num_polarizations,
                        const float *psf, int64_t psf_row_stride, int64_t psf_pol_stride,
                        int psf_width, int psf_height, int patch_width, int patch_height,
                        int border, int mode, float loop_gain, float threshold,
                        float *tile_max, int32_t *tile_pos, int tiles_x, int tiles_y,
                        int max_cycles, int form, void *state, float *log, void *stream,
                        const uint8_t *mask, int64_t mask_row_stride)
{
    KIMG_CHECK_ARG(dirty && model && psf && tile_max && tile_pos && state && log);
    KIMG_CHECK_ARG(num_polarizations >= 1 && num_polarizations <= 4 && max_cycles >= 0);
    KIMG_CHECK_ARG(patch_width > 0 && patch_height > 0 && patch_width <= psf_width
                   && patch_height <= psf_height && tiles_x > 0 && tiles_y > 0);
    KIMG_CHECK_ARG(mode == KIMG_CLEAN_I || mode == KIMG_CLEAN_SUMSQ);
    KIMG_CHECK_ARG(row_stride >= width && psf_row_stride >= psf_width);
    const int components = (form >> 8) & 0xff;      // KIMG_CLEAN_FORM_MULTI: lattices per launch
    // ... and steps per lattice (0: as many as the form takes); bit 4: the repeated-steps kernel from
    // the first launch on, whatever the field looks like (tests)
    const int repeats = (form >> 16) & 0x1f;
    form &= 0xff;
    KIMG_CHECK_ARG(form == KIMG_CLEAN_FORM_AUTO || form == KIMG_CLEAN_FORM_TWO_LAUNCH
                   || form == KIMG_CLEAN_FORM_ONE_LAUNCH || form == KIMG_CLEAN_FORM_PERSISTENT
                   || form == KIMG_CLEAN_FORM_ONE_WORKGROUP || form == KIMG_CLEAN_FORM_MULTI);
    const bool masked = mask != nullptr;
    KIMG_CHECK_ARG(!masked || mask_row_stride >= width);
    // with a mask: two launches or one launch per cycle only (before anything is enqueued)
    if (masked && (form == KIMG_CLEAN_FORM_MULTI || form == KIMG_CLEAN_FORM_PERSISTENT
                   || form == KIMG_CLEAN_FORM_ONE_WORKGROUP))
        return KIMG_EUNSUPPORTED;
    hipStream_t s = (hipStream_t) stream;
    // several components per launch where the patch leaves room for at least two lattices among
    // the 256 records of a launch (a call of a few cycles is not worth the host-paced loop)
    if (!masked) {
        const int m = kimg_clean_multi_components(patch_width, patch_height, tiles_x, tiles_y);
        if (max_cycles > 0 && (form == KIMG_CLEAN_FORM_MULTI ? m >= 1
                                                             : form == KIMG_CLEAN_FORM_AUTO && m >= 2
                                                                   && max_cycles >= 4)) {
            const int rc = kimg_clean_multi_run(
                dirty, model, row_stride, pol_stride, width, height, num_polarizations, psf,
                psf_row_stride, psf_pol_stride, psf_width, psf_height, patch_width, patch_height,
                border, mode, loop_gain, threshold, tile_max, tile_pos, tiles_x, tiles_y,
                max_cycles, components, repeats, false, 0.0, 0.0, state, log, s);
            if (rc != KIMG_EUNSUPPORTED)
                return rc;
        }
        if (form == KIMG_CLEAN_FORM_MULTI)
            form = KIMG_CLEAN_FORM_AUTO;
    }
    // (KIMG_CLEAN_FORM_PERSISTENT and _ONE_WORKGROUP are retired names of the one-launch form)
    const bool fused = patch_fits_one_launch(patch_width, patch_height)
                       && tiles_fit_one_launch(tiles_x, tiles_y) && form != KIMG_CLEAN_FORM_TWO_LAUNCH;
    cycle_args a;
    fill_shared(a, row_stride, pol_stride, width, height, num_polarizations, psf_row_stride,
                psf_pol_stride, psf_width, psf_height, border, mode, loop_gain, tiles_x, tiles_y, fused);
    a.dirty = dirty; a.model = model; a.psf = psf; a.patch_width = patch_width;
    a.patch_height = patch_height; a.tile_max = tile_max; a.tile_pos = tile_pos;
    a.state = static_cast<clean_state *>(state); a.log = log;
    a.mask = mask; a.mask_row_stride = masked ? mask_row_stride : 0;
    int rc = begin_state(a, state, max_cycles, threshold, dirty, tile_pos, s);
    if (rc)
        return rc;
    if (fused)
        begin_owners(a, state, tile_max, tile_pos, s);
    rc = run_cycles(a, max_cycles, s);
    if (rc)
        return rc;
    if (fused)
        end_state(state, tile_max, tile_pos, s);
    return kimg_launch_status();
}

extern "C" int kimg_clean_cycles(float *dirty, float *model, int64_t row_stride,
                                 int64_t pol_stride, int width, int height, int num_polarizations,
                                 const float *psf, int64_t psf_row_stride, int64_t psf_pol_stride,
                                 int psf_width, int psf_height, int patch_width, int patch_height,
                                 int border, int mode, float loop_gain, float threshold,
                                 float *tile_max, int32_t *tile_pos, int tiles_x, int tiles_y,
                                 int max_cycles, int form, void *state, float *log, void *stream)
{
    return clean_cycles(dirty, model, row_stride, pol_stride, width, height, num_polarizations, psf,
                        psf_row_stride, psf_pol_stride, psf_width, psf_height, patch_width,
                        patch_height, border, mode, loop_gain, threshold, tile_max, tile_pos, tiles_x,
                        tiles_y, max_cycles, form, state, log, stream, nullptr, 0);
}

extern "C" int kimg_clean_cycles_masked(float *dirty, float *model, int64_t row_stride,
                                        int64_t pol_stride, int width, int height,
                                        int num_polarizations, const float *psf,
                                        int64_t psf_row_stride, int64_t psf_pol_stride, int psf_width,
                                        int psf_height, int patch_width, int patch_height, int border,
                                        int mode, float loop_gain, float threshold, float *tile_max,
                                        int32_t *tile_pos, int tiles_x, int tiles_y, int max_cycles,
                                        int form, void *state, float *log, void *stream,
                                        const uint8_t *mask, int64_t mask_row_stride)
{
    return clean_cycles(dirty, model, row_stride, pol_stride, width, height, num_polarizations, psf,
                        psf_row_stride, psf_pol_stride, psf_width, psf_height, patch_width,
                        patch_height, border, mode, loop_gain, threshold, tile_max, tile_pos, tiles_x,
                        tiles_y, max_cycles, form, state, log, stream, mask, mask_row_stride);
}

extern "C" int kimg_clean_cycles_batch(const kimg_clean_channel *channels_in, int num_channels,
                                       int64_t row_stride, int64_t pol_stride, int width,
                                       int height, int num_polarizations, int64_t psf_row_stride,
                                       int64_t psf_pol_stride, int psf_width, int psf_height,
                                       int border, int mode, float loop_gain, int tiles_x,
                                       int tiles_y, void *stream)
{
    KIMG_CHECK_ARG(channels_in && num_channels >= 1 && num_channels <= KIMG_CLEAN_BATCH_MAX);
    KIMG_CHECK_ARG(num_polarizations >= 1 && num_polarizations <= 4 && tiles_x > 0 && tiles_y > 0);
    KIMG_CHECK_ARG(mode == KIMG_CLEAN_I || mode == KIMG_CLEAN_SUMSQ);
    KIMG_CHECK_ARG(row_stride >= width && psf_row_stride >= psf_width);
    hipStream_t s = (hipStream_t) stream;
    cycle_args a;
    fill_shared(a, row_stride, pol_stride, width, height, num_polarizations, psf_row_stride,
                psf_pol_stride, psf_width, psf_height, border, mode, loop_gain, tiles_x, tiles_y, true);
    int max_cycles = 0;
    if (!tiles_fit_one_launch(tiles_x, tiles_y))
        return KIMG_EUNSUPPORTED;
    // The order of the channels does not matter to the results, but the captured graph is cached
    // per argument set: channels that meet in another order (threads arriving at a rendezvous)
    // must find the same graph, so the table is kept sorted by image address.
    kimg_clean_channel sorted[KIMG_CLEAN_BATCH_MAX];
    for (int c = 0; c < num_channels; c++) {
        int at = c;
        while (at > 0 && sorted[at - 1].dirty > channels_in[c].dirty) {
            sorted[at] = sorted[at - 1];
            at--;
        }
        sorted[at] = channels_in[c];
    }
    const kimg_clean_channel *channels = sorted;
    for (int c = 0; c < num_channels; c++) {
        const kimg_clean_channel &ch = channels[c];
        KIMG_CHECK_ARG(ch.dirty && ch.model && ch.psf && ch.tile_max && ch.tile_pos && ch.state
                       && ch.log && ch.max_cycles >= 0);
        KIMG_CHECK_ARG(ch.patch_width > 0 && ch.patch_height > 0 && ch.patch_width <= psf_width
                       && ch.patch_height <= psf_height);
        for (int o = 0; o < c; o++)     // channels are cleaned concurrently: no shared buffers
            KIMG_CHECK_ARG(channels[o].dirty != ch.dirty && channels[o].state != ch.state
                           && channels[o].tile_max != ch.tile_max && channels[o].log != ch.log);
        if (!patch_fits_one_launch(ch.patch_width, ch.patch_height))
            return KIMG_EUNSUPPORTED;
        const int bx = kimg_divup(ch.patch_width, TILE) + 1, by = kimg_divup(ch.patch_height, TILE) + 1;
        a.batch_blocks = bx * by > a.batch_blocks ? bx * by : a.batch_blocks;
        max_cycles = ch.max_cycles > max_cycles ? ch.max_cycles : max_cycles;
        batch_channel &b = a.tab.ch[c];
        b.dirty = ch.dirty;
        b.model = ch.model;
        b.psf = ch.psf;
        b.tile_max = ch.tile_max;
        b.tile_pos = ch.tile_pos;
        b.scratch = static_cast<fused_scratch *>(ch.state);
        b.log = ch.log;
        b.patch_w = ch.patch_width;
        b.patch_h = ch.patch_height;
    }
    a.batch = num_channels;
    // per channel, in the order of a single channel's call
    for (int c = 0; c < num_channels; c++) {
        const kimg_clean_channel &ch = channels[c];
        const int rc = begin_state(a, ch.state, ch.max_cycles, ch.threshold, ch.dirty, ch.tile_pos, s);
        if (rc)
            return rc;
        begin_owners(a, ch.state, ch.tile_max, ch.tile_pos, s);
    }
    int rc = kimg_launch_status();
    if (rc == 0)
        rc = run_cycles(a, max_cycles, s);
    if (rc)
        return rc;
    for (int c = 0; c < num_channels; c++)
        end_state(channels[c].state, channels[c].tile_max, channels[c].tile_pos, s);
    return kimg_launch_status();
}

extern "C" int kimg_psf_patch(const float *psf, int64_t row_stride, int64_t pol_stride,
                              int num_polarizations, int min_x, int min_y, int max_x, int max_y,
                              int mid_x, int mid_y, float threshold, int32_t *bound, void *stream)
{
    KIMG_CHECK_ARG(psf && bound && num_polarizations >= 1 && max_x >= min_x && max_y >= min_y);
    KIMG_CHECK_ARG(row_stride > max_x);     // (the call has no width: the region must fit a row)
    hipStream_t s = (hipStream_t) stream;
    KIMG_HIP(hipMemsetAsync(bound, 0, 2 * sizeof(int32_t), s));
    psf_patch_kernel<<<region_grid(max_x - min_x + 1, max_y - min_y + 1), 256, 0, s>>>(
        psf, row_stride, pol_stride, num_polarizations, min_x, min_y, max_x, max_y, mid_x, mid_y,
        threshold, bound);
    return kimg_launch_status();
}

extern "C" int kimg_abs_histogram(const float *image, int64_t row_stride, int64_t pol_stride,
                                  int width, int height, int num_polarizations, int border,
                                  int pass, uint32_t prefix, uint32_t *hist, void *stream)
{
    KIMG_CHECK_ARG(image && hist && pass >= 0 && pass <= 3 && border >= 0);
    KIMG_CHECK_ARG(width > 2 * border && height > 2 * border && num_polarizations >= 1);
    KIMG_CHECK_ARG(row_stride >= width);
    hipStream_t s = (hipStream_t) stream;
    KIMG_HIP(hipMemsetAsync(hist, 0, 256 * sizeof(uint32_t), s));
    abs_histogram_kernel<<<region_grid(width - 2 * border, height - 2 * border, 2048), 256, 0, s>>>(
        image, row_stride, pol_stride, width, height, num_polarizations, border, pass, prefix, hist);
    return kimg_launch_status();
}

extern "C" int kimg_abs_count_le(const float *image, int64_t row_stride, int64_t pol_stride,
                                 int width, int height, int num_polarizations, int border,
                                 float value, uint32_t *out, void *stream)
{
    KIMG_CHECK_ARG(image && out && border >= 0 && num_polarizations >= 1);
    KIMG_CHECK_ARG(width > 2 * border && height > 2 * border && row_stride >= width);
    hipStream_t s = (hipStream_t) stream;
    static const uint32_t init[2] = {0u, 0xffffffffu};
    KIMG_HIP(hipMemcpyAsync(out, init, sizeof(init), hipMemcpyHostToDevice, s));
    union { float f; uint32_t u; } conv;
    conv.f = value;
    const uint32_t bits = conv.u;
    abs_count_le_kernel<<<region_grid(width - 2 * border, height - 2 * border, 4096), 256, 0, s>>>(
        image, row_stride, pol_stride, width, height, num_polarizations, border,
        bits & 0x7fffffffu, out);
    return kimg_launch_status();
}

// ---- whole noise estimate without host round trips ------------------------------------------
namespace {

// The two middle ranks ((n-1)/2 and n/2: the same element for odd n) are resolved side by side,
// so the upper one costs no pass of its own: while both still lie behind the same bytes one
// histogram serves the pair, and from the pass after they part each has its own.
// Workgroups add their histogram into one of NOISE_SLOTS copies: atomics on one address are
// served one after the other (~30 ns each), and 2048 workgroups behind the same few bins of the
// exponent byte were most of a pass.
constexpr int NOISE_SLOTS = 32;
struct noise_state {
    uint32_t prefix[2];     // bytes of the rank's |x| chosen so far
    uint32_t k[2];          // rank still to resolve inside the current prefix
    uint32_t hist[2][NOISE_SLOTS][256];
};

// One radix-select pass over the interior: histogram of byte `pass` of |x|'s bit pattern among
// the pixels whose higher bytes equal the rank's prefix.  TOP: the first pass (the sign-less
// exponent byte, every pixel counts).
template<bool TOP>
__global__ __launch_bounds__(256) void abs_histogram2_kernel(
    const float *__restrict__ image, int64_t row_stride, int64_t pol_stride, int width,
    int height, int P, int border, int pass, noise_state *__restrict__ st)
{
    __shared__ uint32_t local[2][256];
    local[0][threadIdx.x] = 0;
    local[1][threadIdx.x] = 0;
    const uint32_t prefix0 = st->prefix[0], prefix1 = st->prefix[1];
    const bool split = !TOP && prefix0 != prefix1;
    __syncthreads();
    const int shift = TOP ? 24 : 8 * pass;
    // TOP: the exponent byte of a noise-like image takes three or four neighbouring values, and
    // 64 LDS atomics on one address are served one after the other; each thread counts the four
    // values up to the largest of its wave's first row in registers instead (anything else --
    // an image with a wide dynamic range -- still goes to the LDS histogram directly).
    uint32_t base = 0, near[4] = {0, 0, 0, 0};
    bool have_base = false;
    constexpr int ROWS = 4;
    const int x = border + blockIdx.x * blockDim.x + threadIdx.x;
    const bool x_ok = x < width - border;
    for (int p = 0; p < P; p++)
        for (int y0 = border + blockIdx.y; y0 < height - border; y0 += gridDim.y * ROWS) {
            uint32_t keys[ROWS];
            bool ok[ROWS];
#pragma unroll
            for (int r = 0; r < ROWS; r++) {
                const int y = y0 + r * gridDim.y;
                ok[r] = x_ok && y < height - border;
                keys[r] = ok[r] ? __float_as_uint(image[p * pol_stride + (int64_t) y * row_stride + x])
                                      & 0x7fffffffu : 0u;
            }
            if (TOP && !have_base) {
                base = ok[0] ? keys[0] >> 24 : 0u;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1)
                    base = max(base, (uint32_t) __shfl_xor((int) base, off, WAVE));
                have_base = true;
            }
#pragma unroll
            for (int r = 0; r < ROWS; r++) {
                const uint32_t key = keys[r];
                const uint32_t bin = (key >> shift) & 255u;
                if (TOP) {
                    const uint32_t d = base - bin;
                    if (ok[r]) {
#pragma unroll
                        for (int j = 0; j < 4; j++)
                            near[j] += d == (uint32_t) j;
                        if (d > 3u)
                            atomicAdd(&local[0][bin], 1u);
                    }
                } else {
                    const uint32_t upper = key >> (shift + 8);
                    // a mantissa byte: the bins of neighbouring pixels differ
                    if (ok[r] && upper == prefix0)
                        atomicAdd(&local[0][bin], 1u);
                    if (split && ok[r] && upper == prefix1)
                        atomicAdd(&local[1][bin], 1u);
                }
            }
        }
    if (TOP) {
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (near[j])
                atomicAdd(&local[0][base - j], near[j]);
    }
    __syncthreads();
    const int slot = (blockIdx.y * gridDim.x + blockIdx.x) % NOISE_SLOTS;
    if (local[0][threadIdx.x])
        atomicAdd(&st->hist[0][slot][threadIdx.x], local[0][threadIdx.x]);
    if (local[1][threadIdx.x])
        atomicAdd(&st->hist[1][slot][threadIdx.x], local[1][threadIdx.x]);
}

// Pick, for each of the two ranks, the byte whose bin holds it, descend into it, clear the
// histograms for the next pass.
__global__ __launch_bounds__(256) void radix_select2_kernel(noise_state *st, bool last,
                                                            float median_to_rms, float *out)
{
    __shared__ uint32_t cum[256];
    const int t = threadIdx.x;
    const bool split = st->prefix[0] != st->prefix[1];
    const uint32_t k[2] = {st->k[0], st->k[1]};
    const uint32_t prefix[2] = {st->prefix[0], st->prefix[1]};
    __syncthreads();
    uint32_t total[2] = {0, 0};
    for (int r = 0; r < 2; r++)
        for (int slot = 0; slot < NOISE_SLOTS; slot++) {
            total[r] += st->hist[r][slot][t];
            st->hist[r][slot][t] = 0;
        }
    for (int r = 0; r < 2; r++) {
        if (r == 0 || split) {
            const uint32_t mine = total[r];
            __syncthreads();
            cum[t] = mine;
            __syncthreads();
            for (int off = 1; off < 256; off <<= 1) {
                const uint32_t add = t >= off ? cum[t - off] : 0;
                __syncthreads();
                cum[t] += add;
                __syncthreads();
            }
        }
        const uint32_t mine = total[split ? r : 0];
        const uint32_t below = cum[t] - mine;
        if (below <= k[r] && k[r] < cum[t]) {       // exactly one bin
            st->k[r] = k[r] - below;
            st->prefix[r] = (prefix[r] << 8) | (uint32_t) t;
        }
    }
    if (last) {
        __threadfence_block();
        __syncthreads();
        if (t == 0) {
            const volatile uint32_t *chosen = st->prefix;
            const float lo = __uint_as_float(chosen[0]);
            const float hi = __uint_as_float(chosen[1]);
            const float median = (lo + hi) / 2.0f;      // np.median of float32 data (clean.py:942)
            *out = median * median_to_rms;
        }
    }
}

// Clear the histograms and set the two ranks.
__global__ __launch_bounds__(1024) void noise_init_kernel(noise_state *st, uint32_t k0, uint32_t k1)
{
    uint32_t *words = &st->hist[0][0][0];
    for (int i = threadIdx.x; i < 2 * NOISE_SLOTS * 256; i += blockDim.x)
        words[i] = 0;
    if (threadIdx.x == 0) {
        st->prefix[0] = st->prefix[1] = 0;
        st->k[0] = k0;
        st->k[1] = k1;
    }
}

} // namespace

extern "C" size_t kimg_noise_est_scratch_bytes(void) { return sizeof(noise_state); }

extern "C" int kimg_noise_est(const float *image, int64_t row_stride, int64_t pol_stride,
                              int width, int height, int num_polarizations, int border,
                              float median_to_rms, void *scratch, float *out, void *stream)
{
    KIMG_CHECK_ARG(image && scratch && out && border >= 0 && num_polarizations >= 1);
    KIMG_CHECK_ARG(width > 2 * border && height > 2 * border && row_stride >= width);
    const int64_t n64 = (int64_t) (width - 2 * border) * (height - 2 * border) * num_polarizations;
    KIMG_CHECK_ARG(n64 < ((int64_t) 1 << 32));
    const uint32_t n = (uint32_t) n64;
    hipStream_t s = (hipStream_t) stream;
    noise_state *st = static_cast<noise_state *>(scratch);
    noise_init_kernel<<<1, 1024, 0, s>>>(st, (n - 1) / 2, n / 2);    // the middle pair, clean.py:938-943
    const dim3 gh = region_grid(width - 2 * border, height - 2 * border, 2048);
    for (int pass = 3; pass >= 0; pass--) {
        if (pass == 3)
            abs_histogram2_kernel<true><<<gh, 256, 0, s>>>(
                image, row_stride, pol_stride, width, height, num_polarizations, border, pass, st);
        else
            abs_histogram2_kernel<false><<<gh, 256, 0, s>>>(
                image, row_stride, pol_stride, width, height, num_polarizations, border, pass, st);
        radix_select2_kernel<<<1, 256, 0, s>>>(st, pass == 0, median_to_rms, out);
    }
    return kimg_launch_status();
}

// (kimg_preload, api.hip)
KIMG_PRELOAD_THIS_UNIT(subtract_psf_kernel)
