// MFMA window gridder for gfx950 (CDNA4) -- the hot kernel of the path.
//
// Replaces Gridder.static_run / grid.mako:63-197 of the reference for kernel widths <= 64
// (widths above 32 as 2 x 2 tap blocks, see tap_split).
// Same result as GridderHost/_grid (grid.py:1032-1052):
//     grid[p][v0+j][u0+k] += vis[p]*wgt[p] * conj(kern[w][sv][j]) * conj(kern[w][su][k]).
//
// Design (CDNA4-first, not the reference's thread-per-cell Romein kernel):
//  * A wave owns a moving 32x32 window of the grid held in MFMA accumulators
//    (v_mfma_f32_32x32x2_f32: exact fp32, 16 VGPRs for Re + 16 for Im per polarization).
//    Cell (r, c) of the window is grid point (Wv + ((r-Wv)&31), Wu + ((c-Wu)&31)), so the
//    window slides without moving data; cells are flushed with float atomics only when
//    their mapping changes (the window outran them) and once at the end of the wave's range.
//  * A visibility's K x K update is a rank-1 outer product a (x) b with
//    a[j] = vis*wgt*conj(kv[j]), b[k] = conj(ku[k]).  The complex product is folded into ONE
//    real MFMA per 32x16-cell tile: the MFMA K=2 dimension carries (Re a, Im a) and the N
//    dimension carries interleaved (re, im) output columns, B = [[ku.re, -ku.im], [ku.im,
//    ku.re]].  Two tiles cover the 32x32 window: 2 MFMAs per visibility and polarization.
//    All per-tap arithmetic therefore runs on the matrix pipe; the VALU only prepares one A
//    and two B elements per lane per visibility.
//  * The separable kernel table (W x OV rows, padded to 32 taps) lives in LDS when it fits
//    (up to 512 rows); otherwise -- hundreds of W planes, or the two tables of a wide kernel --
//    the operands come from a zero-padded copy in HBM (template flag TG, served by L1/L2).
//    Visibilities are loaded 64 at a time (lane i <-> visibility i, coalesced, two batches
//    prefetched), staged per wave in LDS and read back as broadcasts.  The scalar unit is a
//    scarce resource (one issue slot shared by a SIMD's waves), so the window test runs once
//    per group of 8 visibilities on bounds reduced with DPP; the hot loop is a hand-pipelined
//    sequence of 4-visibility stages (operand reads one stage ahead of 8 back-to-back MFMAs)
//    with no flush code inside.
//  * Accumulator columns are (re, im)-interleaved, so a flush writes 128 contiguous bytes
//    per half-wave -- the shape global float atomics run at full rate for.
//  * Window slack 32-K lets consecutive visibilities whose footprints differ by a few
//    cells share accumulators without any flush.
//
//  * The default float32 form runs the same sums on v_mfma_f32_16x16x4_f32, TWO visibilities per
//    instruction (PAIR: window_acc16, pair32_ops): fewer address and LDS instructions per visibility,
//    8 instructions of 32 cycles per pair instead of 2 x 2 of 64; the 32x32x2 form stays selectable
//    (KIMG_ARITH_FP32_32X32).
//  * Consecutive records with equal (u, v, sub_u, sub_v, w_plane) apply the same rank-1 matrix, so the
//    staging step sums their weighted samples and stages ONE record per run (a ballot for the run
//    heads, a segmented sum over lanes, a compaction through LDS; runs are cut at the ends of a
//    batch of 64).  An uncompressed track stream repeats its predecessor's sub-cell in 6 of 7
//    records; a stream that was merged before takes a scalar branch around the step.
//    KIMG_ARITH_NO_FOLD switches it off.
// Algorithmic work per visibility: 8*K*K*P flop (complex MAC per tap) + 6*K*P (a-vector);
// executed: 2 MFMA x 2048 MAC per visibility per polarization (32x32 window).
#include "kimg_window_launch.h"
#include <limits.h>
#include <string.h>
#include <type_traits>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// Accumulators of one 32x32 window of complex cells, as two MFMA tiles of 32 rows x 16
// complex columns with (re, im) interleaved along the MFMA N dimension:
// tile t, register k, lane l  <->  row (k&3) + 8*(k>>2) + 4*(l>>5),
//                                  complex column ((l&31)>>1) + 16*t, part l&1 (0 re, 1 im).
template <int P>
struct window_acc {
    f32x16 t0[P];
    f32x16 t1[P];
};

// 32-bit mask of the window indices i whose mapping W + ((i - W) & 31) changes when the
// origin moves from W to nW (all of them when |nW - W| >= 32).
__device__ inline uint32_t changed_mask(int W, int nW)
{
    const int d = nW - W;
    if (d == 0)
        return 0u;
    if (d >= WIN || d <= -WIN)
        return 0xffffffffu;
    // forward move: the d lowest offsets wrap forward; backward: the |d| highest wrap back
    const uint32_t offsets = d > 0 ? (1u << d) - 1u : ~((1u << (WIN + d)) - 1u);
    const int rot = W & 31;                         // offset o <-> index (W + o) & 31
    return rot ? (offsets << rot) | (offsets >> (32 - rot)) : offsets;
}

// Flush (atomically add and clear) every accumulator cell whose grid mapping differs
// between window origin (Wu, Wv) and (nWu, nWv); `full` flushes everything.  One wave
// instruction covers two grid rows x 128 contiguous bytes (16 complex cells), the shape
// global float atomics run at full rate for.  Registers whose rows and columns are all
// unaffected are skipped with a scalar test.
//
// Window moves are frequent on fast tracks (every few visibilities for the 30-tap blocks of a wide
// kernel, whose slack is 2 cells), and a wave issues at most one instruction every few cycles, so
// the flush is built for a short INSTRUCTION STREAM: 32-bit byte offsets on a scalar base
// (global_atomic ... s[base]), the grid row of register k as two vector instructions plus one
// multiply-add per tile, and no per-cell test that the kind of move makes unnecessary --
// ROWS says whether row predicates are needed at all (false for the common pure column move),
// and windows that lie wholly inside the grid (nearly all) skip the bounds tests.
// SCALED: multiply by scale[p] on the way out (fp16 form); the float32 form's scale is 1.
template <int P, bool SCALED, bool ROWS, bool COLS, bool BOUNDS>
__device__ __attribute__((always_inline)) inline void flush_cells(
    window_acc<P> &acc, float *__restrict__ grid, unsigned row_bytes, int64_t pol_stride, int Gg,
    int Wu, int Wv, uint32_t row_mask, uint32_t col_mask, int lane, const float (&scale)[P])
{
    const int part = lane & 1;
    const int cx0 = (lane & 31) >> 1;
    const int c = (lane >> 5) * 4 - Wv;             // window row of register k = (rk + c) & 31
    const uint32_t lane_rows = row_mask >> ((lane >> 5) * 4);   // bit rk <-> this lane's row of register k
    unsigned base[2];
    bool col_sel[2];
#pragma unroll
    for (int t = 0; t < 2; t++) {
        const int cx = cx0 + 16 * t;
        const int xold = Wu + ((cx - Wu) & 31);
        base[t] = (unsigned) Wv * row_bytes + (unsigned) (2 * xold + part) * 4u;   // (wraps like the sum)
        col_sel[t] = COLS ? ((col_mask >> cx) & 1u) != 0 : false;
        if (BOUNDS && (unsigned) xold >= (unsigned) Gg)
            base[t] = 0xffffffffu;                  // marks a column outside the grid
    }
#pragma unroll
    for (int k = 0; k < 16; k++) {
        constexpr uint32_t one = 1u;
        const int rk = (k & 3) + 8 * (k >> 2);          // MFMA 32x32 C/D row of register k (lower half)
        if (ROWS && !COLS && (row_mask & ((one << rk) | (one << (rk + 4)))) == 0)
            continue;                                   // uniform: nothing of register k moves
        const unsigned rr = (unsigned) (rk + c) & 31u;
        const bool row_sel = ROWS ? ((lane_rows >> rk) & 1u) != 0 : false;
        const bool y_ok = BOUNDS ? (unsigned) (Wv + (int) rr) < (unsigned) Gg : true;
#pragma unroll
        for (int t = 0; t < 2; t++) {
            const bool sel = (ROWS || COLS) ? (row_sel || col_sel[t]) : true;
            const unsigned off = rr * row_bytes + base[t];      // v_mad_u32_u24
            const bool inside = BOUNDS ? (y_ok && base[t] != 0xffffffffu) : true;
#pragma unroll
            for (int p = 0; p < P; p++) {
                const float v = t ? acc.t1[p][k] : acc.t0[p][k];
                if (sel && inside && v != 0.0f) {
                    float *cell = reinterpret_cast<float *>(
                        reinterpret_cast<char *>(grid + 2 * p * pol_stride) + off);
                    atomicAdd(cell, SCALED ? v * scale[p] : v);
                }
                if (t)
                    acc.t1[p][k] = sel ? 0.0f : v;
                else
                    acc.t0[p][k] = sel ? 0.0f : v;
            }
        }
    }
}

// Accumulators of the pair form (float32, v_mfma_f32_16x16x4_f32, two visibilities per instruction):
// the same 32x32 window as 2 x 4 tiles of 16 rows x 8 complex columns, tile 4 rb + cb covering
// rows 16 rb .. 16 rb + 15 and complex columns 8 cb .. 8 cb + 7:
// tile t, register k, lane l  <->  row 16 (t >> 2) + 4 (l >> 4) + k,
//                                  complex column 8 (t & 3) + ((l & 15) >> 1), part l & 1.
template <int P>
struct window_acc16 {
    f32x4 t[P][8];
};

// flush_cells for the pair form's layout.  One wave instruction covers four grid rows x 64
// contiguous bytes; a register whose rows (a move along v) or whose columns (a move along u) are
// all unaffected is skipped with a scalar test.
template <int P, bool SCALED, bool ROWS, bool COLS, bool BOUNDS>
__device__ __attribute__((always_inline)) inline void flush_cells(
    window_acc16<P> &acc, float *__restrict__ grid, unsigned row_bytes, int64_t pol_stride, int Gg,
    int Wu, int Wv, uint32_t row_mask, uint32_t col_mask, int lane, const float (&scale)[P])
{
    const int part = lane & 1;
    const int cx0 = (lane & 15) >> 1;
    const int c = (lane >> 4) * 4 - Wv;             // window row of register k of row block rb = (16 rb + k + c) & 31
    const uint32_t lane_rows = row_mask >> ((lane >> 4) * 4);   // bit 16 rb + k <-> this lane's row
    unsigned base[4];
    bool col_sel[4];
#pragma unroll
    for (int cb = 0; cb < 4; cb++) {
        const int cx = cx0 + 8 * cb;
        const int xold = Wu + ((cx - Wu) & 31);
        base[cb] = (unsigned) Wv * row_bytes + (unsigned) (2 * xold + part) * 4u;   // (wraps like the sum)
        col_sel[cb] = COLS ? ((col_mask >> cx) & 1u) != 0 : false;
        if (BOUNDS && (unsigned) xold >= (unsigned) Gg)
            base[cb] = 0xffffffffu;                 // marks a column outside the grid
    }
#pragma unroll
    for (int rb = 0; rb < 2; rb++)
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int rk = 16 * rb + k;                     // row of register k for lanes 0-15
        if (ROWS && !COLS && (row_mask & (0x1111u << rk)) == 0)
            continue;                                   // uniform: nothing of these registers moves
        const unsigned rr = (unsigned) (rk + c) & 31u;
        const bool row_sel = ROWS ? ((lane_rows >> rk) & 1u) != 0 : false;
        const bool y_ok = BOUNDS ? (unsigned) (Wv + (int) rr) < (unsigned) Gg : true;
#pragma unroll
        for (int cb = 0; cb < 4; cb++) {
            if (COLS && !ROWS && ((col_mask >> (8 * cb)) & 0xffu) == 0)
                continue;                               // uniform: none of the tile's columns moves
            const bool sel = (ROWS || COLS) ? (row_sel || col_sel[cb]) : true;
            const unsigned off = rr * row_bytes + base[cb];
            const bool inside = BOUNDS ? (y_ok && base[cb] != 0xffffffffu) : true;
#pragma unroll
            for (int p = 0; p < P; p++) {
                const float v = acc.t[p][4 * rb + cb][k];
                if (sel && inside && v != 0.0f) {
                    float *cell = reinterpret_cast<float *>(
                        reinterpret_cast<char *>(grid + 2 * p * pol_stride) + off);
                    atomicAdd(cell, SCALED ? v * scale[p] : v);
                }
                acc.t[p][4 * rb + cb][k] = sel ? 0.0f : v;
            }
        }
    }
}

template <int P, bool SCALED, class ACC>
__device__ __attribute__((always_inline)) inline void flush_window(
    ACC &acc, float *__restrict__ grid, int64_t row_stride, int64_t pol_stride,
    int Gg, int Wu, int Wv, int nWu, int nWv, bool full, int lane, const float (&scale)[P])
{
    const uint32_t row_mask = full ? 0xffffffffu : changed_mask(Wv, nWv);
    const uint32_t col_mask = full ? 0xffffffffu : changed_mask(Wu, nWu);
    if ((row_mask | col_mask) == 0)
        return;
    const unsigned row_bytes = (unsigned) row_stride * 8u;  // (grid_size * row_bytes < 2^32: checked on the host)
    const bool inside = Wu >= 0 && Wv >= 0 && Wu + WIN <= Gg && Wv + WIN <= Gg;
#define KIMG_FLUSH(ROWS, COLS, BOUNDS) flush_cells<P, SCALED, ROWS, COLS, BOUNDS>( \
        acc, grid, row_bytes, pol_stride, Gg, Wu, Wv, row_mask, col_mask, lane, scale)
    // the two common moves of a window inside the grid get their own short code; everything else
    // (both axes at once, jumps and other full flushes, windows at the grid's rim) the general form
    if (inside && !full && row_mask == 0)
        KIMG_FLUSH(false, true, false);         // along u only
    else if (inside && !full && col_mask == 0)
        KIMG_FLUSH(true, false, false);         // along v only
    else
        KIMG_FLUSH(true, true, true);
#undef KIMG_FLUSH
}

template <int P>
struct vis_raw {
    int2 uv;
    int wp;
    float2 v[P];
    float w[P];
};

typedef float v2f __attribute__((ext_vector_type(2)));

constexpr int GROUP = 8;        // visibilities sharing one window check
constexpr int GROUP_COUNT = 64 / GROUP;
// LDS kernel-table rows hold 32 zero-padded taps.  When the LDS budget allows, each row is
// stored twice (ROW = 64) so that tap (lane - first_tap) mod 32 is a plain "lane + offset"
// address; otherwise (ROW = 32) the wrap costs two more VALU operations per address.

// Operands of SUB staged visibilities (LDS reads in flight or landed):
// c = (Re s, Im s) for lanes 0-31, (Im s, -Re s) for lanes 32-63, so that a = c . kv gives
// Re(s conj kv) resp. Im(s conj kv); kv = this lane's row tap; b0/b1 = this lane's column
// tap component (re or im, chosen by the lane's address) for the two tiles.
template <int P, int SUB>
struct sub_ops {
    float2 c[P][SUB];
    float2 kv[SUB];
    v2f b[SUB];             // (tile 0, tile 1) column operand: adjacent registers for v_pk_mul_f32
};

// min / max over each aligned group of 8 lanes with DPP (VALU rate, no LDS round trips)
__device__ inline int group8_min(int v)
{
    v = min(v, __builtin_amdgcn_mov_dpp(v, 0xB1, 0xf, 0xf, true));     // quad_perm [1,0,3,2]
    v = min(v, __builtin_amdgcn_mov_dpp(v, 0x4E, 0xf, 0xf, true));     // quad_perm [2,3,0,1]
    v = min(v, __builtin_amdgcn_mov_dpp(v, 0x141, 0xf, 0xf, true));    // row_half_mirror
    return v;
}

__device__ inline int group8_max(int v)
{
    v = max(v, __builtin_amdgcn_mov_dpp(v, 0xB1, 0xf, 0xf, true));
    v = max(v, __builtin_amdgcn_mov_dpp(v, 0x4E, 0xf, 0xf, true));
    v = max(v, __builtin_amdgcn_mov_dpp(v, 0x141, 0xf, 0xf, true));
    return v;
}

// TWO: an off-diagonal tap block of a kernel wider than 32 (tap_split, kimg_window_launch.h), with
// a table for the row taps and one for the column taps; such a launch always reads them from HBM.
// TG: the padded table(s) do not fit LDS (many W planes: the reference's default w-step gives
// hundreds per slice) and are read from a zero-padded copy in HBM instead ([rows][32] taps,
// built per call by pad_table_kernel / pad_table_f16_kernel; served by L1/L2 -- rows recur along a track).  Everything
// else is unchanged; only the operand reads are global loads.
// ---- fp16 hi/lo formulation (F16 = true) ------------------------------------------------------
// Each fp32 operand x is carried as two halfs, hi = fp16(x) and lo = fp16(x - hi) (22 bits), and
// a product as hi*hi + hi*lo + lo*hi (the dropped lo*lo is 2^-22 of it).  A complex multiply-add
// therefore needs 6 of the 16 k-slots of v_mfma_f32_32x32x16_f16, so ONE instruction (8 passes)
// carries TWO visibilities -- lanes 0-31 (k 0..7) hold one, lanes 32-63 (k 8..15) the other --
// against one visibility per 16-pass v_mfma_f32_32x32x2_f32: a quarter of the matrix time.
// fp16 has little exponent range, so the operands are scaled by powers of two (exact): the table
// by S (largest tap -> [2^13, 2^14)), the samples of a wave by T (largest sample -> [1, 2)); the
// accumulators then hold grid * S*S*T and are multiplied by 1/(S*S*T) when they are flushed.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// (lo | hi << 16), rounded to nearest (v_cvt_pk_f16_f32): truncation would bias every product
// the same way.  (The name dates from a first version that truncated.)
__device__ inline unsigned cvt_pk_f16_rtz(float lo, float hi)
{
    typedef float pk2f __attribute__((ext_vector_type(2)));
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const pk2f x = {lo, hi};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(x, h2));
}

__device__ inline float f16_bits_to_f32(unsigned bits16)
{
    return (float) __builtin_bit_cast(_Float16, (unsigned short) bits16);
}

// x -> (hi | lo << 16)
__device__ inline unsigned split_f16(float x)
{
    const unsigned hi = cvt_pk_f16_rtz(x, 0.0f) & 0xffffu;
    const float rest = x - f16_bits_to_f32(hi);
    const unsigned lo = cvt_pk_f16_rtz(rest, 0.0f) & 0xffffu;
    return hi | (lo << 16);
}

// (hi | lo << 16) -> fp32
__device__ inline float join_f16(unsigned packed)
{
    return f16_bits_to_f32(packed & 0xffffu) + f16_bits_to_f32(packed >> 16);
}

// A complex tap as it is kept in the tables of the fp16 form: (re_hi | im_hi << 16, re_lo | im_lo << 16)
__device__ inline uint2 split_tap(float re, float im)
{
    const unsigned hi = cvt_pk_f16_rtz(re, im);
    const unsigned lo = cvt_pk_f16_rtz(re - f16_bits_to_f32(hi & 0xffffu), im - f16_bits_to_f32(hi >> 16));
    return make_uint2(hi, lo);
}

// Operands of SUBP staged PAIRS of visibilities (this lane's member of each pair)
template <int P, int SUBP>
struct pair_ops {
    float4 c[P][SUBP];      // (Re s, Im s, Im s, -Re s) * T
    uint2 kv[SUBP];         // row tap: (re_hi | im_hi << 16, re_lo | im_lo << 16), times S
    uint2 t0[SUBP], t1[SUBP];   // column taps of the two tiles, same format
};

#ifdef KIMG_GRID_TIMING
// (test builds only) per-wave {first, last} wall_clock64 of the last launch
__device__ long long *g_timing = nullptr;
#endif

// Operands of SUBP staged pairs of visibilities in the pair form (float32, v_mfma_f32_16x16x4_f32):
// lane l serves member l >> 5 of a pair and the MFMA k index (l >> 4) & 1 (Re / Im of a).
// c = (Re s, Im s) for k even, (Im s, -Re s) for k odd; kv = the row taps of the two row blocks
// (16 taps apart); b = the column tap components of the four column blocks (8 taps apart) as two
// (adjacent-register) pairs for v_pk_mul_f32.
template <int P, int SUBP>
struct pair32_ops {
    float2 c[P][SUBP];
    v2f kv[SUBP][2];
    v2f b[SUBP][2];
};

// (512 until round 3; 384 measures 3-4 % faster on launches of ~7 M records -- a W-slice of the
// re-ordered resident store, where a wave only gets four or five chunks and the tail of the launch
// is one chunk long -- and the same on 50 M-record launches, whose chunks the cap below sets)
#ifndef KIMG_INTERLEAVE_MIN_CHUNK
#define KIMG_INTERLEAVE_MIN_CHUNK 384
#endif
#ifndef KIMG_INTERLEAVE_MAX_PARTS
#define KIMG_INTERLEAVE_MAX_PARTS 16
#endif
constexpr int64_t INTERLEAVE_MIN_CHUNK = KIMG_INTERLEAVE_MIN_CHUNK;     // visibilities: bounds the extra window flushes
constexpr int64_t INTERLEAVE_MAX_PARTS = KIMG_INTERLEAVE_MAX_PARTS;

// The window kernel proper: what one workgroup does with the stream it is given (grid_mfma_kernel
// below decides which stream that is).
template <int P, int NW, int SUB, int ROW, bool TWO, bool TG = false, bool F16 = false,
          bool PAIR = false>
__device__ __attribute__((always_inline)) inline void grid_mfma_body(
    float *__restrict__ grid, int64_t row_stride, int64_t pol_stride, int Gg,
    const float *__restrict__ weights_grid, int64_t wg_row_stride, int64_t wg_pol_stride,
    const int16_t *__restrict__ uv, const int16_t *__restrict__ w_plane,
    const float2 *__restrict__ vis, int64_t num_vis,
    const float2 *__restrict__ kern, int W, int OV, tap_split ts, int64_t vis_per_block,
    int p_total, int dbg, const unsigned char *__restrict__ padded,
    const unsigned *__restrict__ tab_max, int64_t chunk, int64_t scramble, unsigned long long *queue)
{
#ifdef KIMG_GRID_TIMING
    const long long t_begin = wall_clock64();
#endif
    static_assert(!TWO || TG, "two tables are read from HBM");
    static_assert(!F16 || SUB % 2 == 0, "fp16 form: visibilities go in pairs");
    static_assert(!PAIR || (!F16 && SUB % 2 == 0), "pair form: float32, visibilities go in pairs");
    extern __shared__ __align__(16) unsigned char smem[];
    const int table_rows = W * OV;
    const int table_bytes = table_rows * ROW * (int) sizeof(float2);
    const int u_table = TWO ? table_bytes : 0;           // byte offset of the column-tap table
    unsigned char *rec_base = smem + (TG ? 0 : (size_t) table_bytes);
    // wave index: uniform by construction, but the compiler must be told (readfirstlane),
    // or every loop below is lowered to divergent (exec-masked) control flow
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    // per-wave staging of one batch of 64 visibilities:
    //   recs[64]       = byte offsets into the table of (row tu, tap (-mu) mod 32) and
    //                    (row tv, tap (-mv) mod 32)
    //   samples[P][64] = s = vis * density weight as (Re, Im, Im, -Re)
    //   origins[64]    = first-tap grid coordinates (mu, mv), used only when a group jumps
    int2 *recs = reinterpret_cast<int2 *>(rec_base) + wib * 64;
    float4 *samples = reinterpret_cast<float4 *>(rec_base + (size_t) NW * 64 * sizeof(int2))
                      + wib * 64 * P;
    int2 *origins = reinterpret_cast<int2 *>(rec_base + (size_t) NW * 64 * (sizeof(int2) + P * sizeof(float4)))
                    + wib * 64;
    const unsigned char *tbytes = TG ? padded : smem;

    // This wave's contiguous range.
    const int64_t block_start = (int64_t) blockIdx.x * vis_per_block;
    int64_t block_end = block_start + vis_per_block;
    if (block_end > num_vis)
        block_end = num_vis;
    const int64_t span = block_end > block_start ? block_end - block_start : 0;
    // The waves of a SIMD (wave index mod 4) get spans of unequal length, (100 - q) : 100 : (100 + q)
    // percent for the three waves of a 12-wave block (dbg bits 8-15; 0 = equal spans), capped at
    // about one batch of 64 visibilities for long spans.  The SIMD's total work is unchanged, but
    // its waves reach their end flush -- a burst of float atomics limited by the CU's atomic rate --
    // at different times, so that part of it overlaps the remaining waves' arithmetic.  (Measured
    // at 341 visibilities per wave: 89.5 -> 81 us per launch with q = 12, i.e. spans of 4-6 batches.)
    int stagger = (dbg >> 8) & 0xff;
    if (NW != 12)
        stagger = 0;
    else if (span > 0 && (int64_t) stagger * span > 100 * 64 * NW)
        stagger = (int) (100 * 64 * NW / span);         // about one batch per wave at most
    auto wave_edge = [&](int w) {
        int64_t cum = 0;                        // cumulative weight of waves [0, w)
        for (int i = 0; i < w; i++)
            cum += 100 + stagger * ((i >> 2) - 1);
        return span * cum / (100 * NW) / 64 * 64;
    };
    const int64_t start = block_start + wave_edge(wib);
    const int64_t end = wib == NW - 1 ? block_end : block_start + wave_edge(wib + 1);

    // What a wave grids.  chunk == 0: the contiguous range [start, end) above.  chunk > 0 (long
    // launches): the stream is cut into chunks of `chunk` visibilities (a multiple of 64); a wave
    // starts with the chunk of its own number and then takes the next free one from a counter in
    // device memory (`queue`), until none is left.  With one contiguous range per wave the launch
    // ends in a long tail: the three waves of a SIMD do not advance at the same pace (the oldest
    // wave wins the arbitration for the matrix pipe), so the first is done after 72 % of the
    // launch and the last runs alone for the final 13 % -- at a fraction of the SIMD's rate.  Taking
    // work by the chunk keeps all waves busy to the end; a chunk's end costs what a baseline
    // boundary costs, one window flush.  Without a counter (`queue` null: no workspace given) wave g
    // takes chunks g, g + waves, g + 2 waves, ... instead.
    struct batch_pos {
        int64_t b, e;       // first visibility of the batch; end of its chunk (b >= e: no batch)
    };
    const int64_t wave_id = (int64_t) blockIdx.x * NW + wib, waves = (int64_t) gridDim.x * NW;
    // Ticket t is chunk (t * scramble) mod chunks_total (scramble is coprime to the number of chunks):
    // the chunks in flight at any moment are spread over the whole stream.  Neighbouring chunks are
    // neighbouring pieces of one baseline's track, and waves that flush their windows into the same
    // region of the grid at the same time contend for the same cache lines in L2 (measured: handing
    // out the first 85 % of a launch in 8 x longer chunks, in stream order, costs 4 %; gridding a
    // stream that was physically interleaved gains 10 %).
    const int64_t chunks_total = chunk > 0 ? (num_vis + chunk - 1) / chunk : 0;
    auto chunk_pos = [&](int64_t t) __attribute__((always_inline)) {
        batch_pos p;
        const int64_t c = t < chunks_total ? (int64_t) ((unsigned long long) t * (unsigned long long) scramble
                                                        % (unsigned long long) chunks_total) : 0;
        p.b = t < chunks_total ? c * chunk : 0;
        p.e = t < chunks_total ? (p.b + chunk < num_vis ? p.b + chunk : num_vis) : 0;
        return p;
    };
    // the ticket for the chunk after the current one is drawn when the current one is entered, and
    // only looked at when it is left (the atomic's round trip is off the critical path)
    unsigned long long ticket = 0;          // lane 0: value returned by the last draw
    int64_t static_next = wave_id + waves;
    auto draw = [&]() __attribute__((always_inline)) {
        if (queue != nullptr) {
            if (lane == 0)
                ticket = atomicAdd(queue, 1ull);
        } else {
            ticket = (unsigned long long) static_next;
            static_next += waves;
        }
    };
    auto drawn = [&]() __attribute__((always_inline)) {
        const unsigned lo = (unsigned) __builtin_amdgcn_readfirstlane((int) (unsigned) ticket);
        const unsigned hi = (unsigned) __builtin_amdgcn_readfirstlane((int) (unsigned) (ticket >> 32));
        const int64_t t = (int64_t) (((unsigned long long) hi << 32) | lo);
        return queue != nullptr ? t + waves : t;
    };
    auto next_pos = [&](const batch_pos &p) __attribute__((always_inline)) {
        batch_pos n = p;
        n.b = p.b + 64;
        if (n.b >= p.e && chunk > 0 && p.b < p.e) {
            n = chunk_pos(drawn());
            if (n.b < n.e)
                draw();
        }
        return n;
    };
    batch_pos p0;
    if (chunk > 0) {
        p0 = chunk_pos(wave_id);
        draw();
    } else {
        p0.b = start;
        p0.e = end;
    }
    batch_pos p1 = next_pos(p0), p2 = next_pos(p1);

    auto load_raw = [&](const batch_pos &pos, vis_raw<P> &raw) __attribute__((always_inline)) {
        const int64_t b = pos.b, end = pos.e;
        int64_t ii = b + lane;
        ii = ii < end ? ii : end - 1;
        raw.uv = reinterpret_cast<const int2 *>(uv)[ii];
        raw.wp = w_plane[ii];
#pragma unroll
        for (int p = 0; p < P; p++)
            raw.v[p] = vis[ii * p_total + p];
    };
    const int half = Gg / 2;
    auto coords_ok = [&](const batch_pos &pos, const vis_raw<P> &raw) __attribute__((always_inline)) {
        const int u = (short) (raw.uv.x & 0xffff), v = (short) (raw.uv.x >> 16);
        const int su = (short) (raw.uv.y & 0xffff), sv = (short) (raw.uv.y >> 16);
        return pos.b + lane < pos.e && (unsigned) (u + half) < (unsigned) Gg
               && (unsigned) (v + half) < (unsigned) Gg && (unsigned) su < (unsigned) OV
               && (unsigned) sv < (unsigned) OV && (unsigned) raw.wp < (unsigned) W;
    };
    auto gather = [&](const batch_pos &b, vis_raw<P> &raw) __attribute__((always_inline)) {
        const int u = (short) (raw.uv.x & 0xffff), v = (short) (raw.uv.x >> 16);
        const int64_t wa = coords_ok(b, raw) ? (int64_t) (v + half) * wg_row_stride + (u + half) : 0;
#pragma unroll
        for (int p = 0; p < P; p++)
            raw.w[p] = weights_grid[wa + p * wg_pol_stride];
    };

    // Two-deep prefetch of the visibility stream: issue the first loads before staging the
    // kernel table so that their latency hides behind it.
    vis_raw<P> r0, r1;
    const bool active = p0.b < p0.e;
    if (active) {
        load_raw(p0, r0);
        if (p1.b < p1.e)
            load_raw(p1, r1);
        else
            r1 = r0;
    }

    // Stage the kernel table(s): taps [tap0, tap0 + Kp) of every row, zero-padded to 32 taps
    // (and stored twice when ROW == 64).  Two taps (16 bytes) per thread when alignment allows.
    auto stage_table = [&](unsigned char *dst, int tap0, int Kp) __attribute__((always_inline)) {
        if (((ts.K | tap0 | Kp) & 1) == 0) {
            const float4 *kern2 = reinterpret_cast<const float4 *>(kern);
            float4 *table2 = reinterpret_cast<float4 *>(dst);
            // all of a thread's loads are issued before its first LDS write: one L2 round trip
            // instead of one per iteration
            constexpr int STG = 6;
            const int total = table_rows * 16;
            for (int base = threadIdx.x; base < total; base += NW * 64 * STG) {
                float4 v[STG];
#pragma unroll
                for (int i = 0; i < STG; i++) {
                    const int idx = base + i * NW * 64;
                    const int row = idx >> 4, t2 = idx & 15;
                    v[i] = (idx < total && 2 * t2 < Kp)
                               ? kern2[(((int64_t) row * ts.K + tap0) >> 1) + t2]
                               : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                }
#pragma unroll
                for (int i = 0; i < STG; i++) {
                    const int idx = base + i * NW * 64;
                    const int row = idx >> 4, t2 = idx & 15;
                    if (idx < total) {
                        table2[row * (ROW / 2) + t2] = v[i];
                        if (ROW == 64)
                            table2[row * (ROW / 2) + 16 + t2] = v[i];
                    }
                }
            }
        } else {
            float2 *table = reinterpret_cast<float2 *>(dst);
            for (int idx = threadIdx.x; idx < table_rows * ROW; idx += NW * 64) {
                const int row = idx / ROW, t = idx & 31;
                table[idx] = t < Kp ? kern[(int64_t) row * ts.K + tap0 + t] : make_float2(0.0f, 0.0f);
            }
        }
    };
    if (!TG)
        stage_table(smem, ts.tv0, ts.Kv);
    __syncthreads();
    float S_scale = 1.0f;
    if (F16 && TG) {
        // table in HBM: already split by pad_table_f16_kernel, with S from the same maximum
        const unsigned m = *tab_max;
        const int e = (int) (m >> 23) - 127;
        S_scale = m ? __uint_as_float((unsigned) (13 - e + 127) << 23) : 1.0f;
    } else if (F16) {
        // largest |component| of the table -> S, then every tap is split in place
        unsigned *s_tabmax = reinterpret_cast<unsigned *>(rec_base);   // (staging area, not yet in use)
        const unsigned *words = reinterpret_cast<const unsigned *>(smem);
        const int nwords = table_bytes / 4;
        unsigned m = 0;
        for (int i = threadIdx.x; i < nwords; i += NW * 64)
            m = max(m, words[i] & 0x7fffffffu);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
            m = max(m, (unsigned) __shfl_xor((int) m, off, WAVE));
        if (lane == 0)
            s_tabmax[wib] = m;
        __syncthreads();
        for (int w = 0; w < NW; w++)
            m = max(m, s_tabmax[w]);
        // m in [2^e, 2^(e+1)): S = 2^(13 - e)
        const int e = (int) (m >> 23) - 127;
        S_scale = m ? __uint_as_float((unsigned) (13 - e + 127) << 23) : 1.0f;
        uint2 *taps = reinterpret_cast<uint2 *>(smem);
        for (int i = threadIdx.x; i < nwords / 2; i += NW * 64) {
            const uint2 t = taps[i];
            taps[i] = split_tap(__uint_as_float(t.x) * S_scale, __uint_as_float(t.y) * S_scale);
        }
        __syncthreads();
    }
    if (!active)
        return;
    gather(p0, r0);

    const int uv_bias = (ts.K - 1) / 2 - Gg / 2;        // grid.py:1038
    const int Su = WIN - ts.Ku, Sv = WIN - ts.Kv;       // window slack along u and v
    const bool h = lane >= 32;                          // MFMA k index of this lane
    const int part = lane & 1;                          // 0: real part column, 1: imaginary
    // B operand: k=0 pairs with Re(a): (ku.re, -ku.im); k=1 with Im(a): (ku.im, ku.re).
    // Which component a lane needs is folded into its table address, the sign is one VALU op.
    const bool b_take_im = (h != (part != 0));
    const float b_sign = (part && !h) ? -1.0f : 1.0f;
    const int lane_v = (lane & 31) * 8;                                 // row tap, bytes
    const int lane_u = ((lane & 31) >> 1) * 8 + (b_take_im ? 4 : 0);    // column tap component
    const int lane_s = h ? 8 : 0;                                       // (Re,Im) or (Im,-Re)
    const unsigned lds_base = (unsigned) (uintptr_t) (__attribute__((address_space(3))) unsigned char *) smem;
    const uint64_t lane_uv = ((uint64_t) (lds_base + (unsigned) lane_v) << 32) | (lds_base + (unsigned) lane_u);
    // fp16 form: which member of a pair this lane serves, the (whole) column tap it reads, and how
    // its 6 k-slots come from the tap (re_hi, im_hi | re_lo, im_lo): even columns (real part of the
    // result) take (re_hi, im_hi, re_lo, im_lo, re_hi, im_hi) as stored, odd ones (-im_hi, re_hi,
    // -im_lo, re_lo, -im_hi, re_hi); the row operand is (re_hi, im_hi, re_hi, im_hi, re_lo, im_lo)
    const int member = lane >> 5;
    const int lane_u16 = ((lane & 31) >> 1) * 8;
    // pair form: the same per lane, with the MFMA k index (l >> 4) & 1 in place of h, row tap l & 15 of
    // the first row block, column tap (l & 15) >> 1 of the first column block
    const bool pk = ((lane >> 4) & 1) != 0;
    const bool pb_take_im = (pk != (part != 0));
    const float pb_sign = (part && !pk) ? -1.0f : 1.0f;
    const int lane_pv = (lane & 15) * 8;
    const int lane_pu = ((lane & 15) >> 1) * 8 + (pb_take_im ? 4 : 0);
    const int lane_ps = pk ? 8 : 0;
    const uint64_t lane_puv = ((uint64_t) (lds_base + (unsigned) lane_pv) << 32) | (lds_base + (unsigned) lane_pu);
    const unsigned sel = part ? 0x01000302u : 0x03020100u;      // odd columns swap (re, im)
    const unsigned flip = part ? 0x00008000u : 0u;              // ... and negate im
    // fp16 form: per-polarization sample scale T = 2^-E, kept as the integer E so that every decision
    // about it is scalar integer work (gfx950 has no scalar float compare).  E_cur = scale of what
    // the accumulators hold, E_stage = the scale the staging code last gave to a group,
    // out_scale = 1 / (S S T) = 2^E / S^2.
    constexpr int E_NONE = 0x7fff;      // no sample seen yet
    constexpr int E_WIDE = 0x7ffe;      // (per group) staged unscaled: one visibility at a time
    int E_cur[P], E_stage[P];
    float out_scale[P];
#pragma unroll
    for (int p = 0; p < P; p++) {
        E_cur[p] = E_stage[p] = E_NONE;
        out_scale[p] = 1.0f;
    }
    // A group (8 visibilities) keeps the scale of its predecessor while its largest sample, times
    // that scale, stays within [2^-6, 2) (density weights that differ by an order of magnitude
    // between neighbouring cells must not cost a flush per cell); otherwise the window is flushed and a new scale chosen
    // (both ways: a run of small samples after a large one gets its own scale).  A group whose own
    // samples spread over more than 2^11 is handled one visibility at a time; such a visibility
    // keeps the current scale while it stays within [2^-14, 2) of it (the same lower end as the
    // smallest member of an ordinary group: its row operand still has 17 good bits on the weakest
    // tap that matters), so that an occasional tiny sample costs no flush.
#ifndef KIMG_T_SPREAD
#define KIMG_T_SPREAD 11
#endif
    constexpr int T_SPREAD = KIMG_T_SPREAD;
    auto sample_exponent = [](unsigned bits) {      // |x| in [2^e, 2^(e+1)) -> e, clamped
        const int e = (int) (bits >> 23) - 127;
        return e < -100 ? -100 : (e > 100 ? 100 : e);
    };
    auto keeps_scale = [&](int e, int E, int low = -6) {    // 2^e * 2^-E within [2^low, 2)
        return E != E_NONE && e - E <= 0 && e - E >= low;
    };

    typename std::conditional<PAIR, window_acc16<P>, window_acc<P>>::type acc;
    if constexpr (PAIR) {
#pragma unroll
        for (int p = 0; p < P; p++)
            for (int t = 0; t < 8; t++)
                for (int k = 0; k < 4; k++)
                    acc.t[p][t][k] = 0.0f;
    } else {
#pragma unroll
    for (int p = 0; p < P; p++)
        for (int k = 0; k < 16; k++) {
            acc.t0[p][k] = 0.0f;
            acc.t1[p][k] = 0.0f;
        }
    }
    bool have = false;
    int Wu = 0, Wv = 0;

    // Move the window so that [lo_u, hi_u] x [lo_v, hi_v] (first-tap coordinates) fits.
    auto fit_window = [&](int lo_u, int hi_u, int lo_v, int hi_v) __attribute__((always_inline)) {
        if (!have) {
            Wu = lo_u - (Su - (hi_u - lo_u)) / 2;
            Wv = lo_v - (Sv - (hi_v - lo_v)) / 2;
            have = true;
            return;
        }
        const bool bad_u = lo_u < Wu || hi_u > Wu + Su;
        const bool bad_v = lo_v < Wv || hi_v > Wv + Sv;
        if (!(bad_u || bad_v))
            return;
        // leave all the slack ahead in the direction of travel (tracks are smooth curves)
        const int nWu = !bad_u ? Wu : (hi_u > Wu + Su ? lo_u : hi_u - Su);
        const int nWv = !bad_v ? Wv : (hi_v > Wv + Sv ? lo_v : hi_v - Sv);
        const bool full = nWu - Wu >= WIN || Wu - nWu >= WIN || nWv - Wv >= WIN || Wv - nWv >= WIN;
        if (!(dbg & 2))
            flush_window<P, F16>(acc, grid, row_stride, pol_stride, Gg, Wu, Wv, nWu, nWv, full, lane,
                            out_scale);
        Wu = nWu;
        Wv = nWv;
    };

    // LDS byte addresses of this lane's row tap / column tap for a staged record
    // (unsigned: with the table in HBM the 32-bit offset then rides on the scalar base pointer
    // -- global_load v, v_off, s[base] -- instead of costing a sign extension and a 64-bit add)
    auto addr_v = [&](int ry) __attribute__((always_inline)) {
        return (unsigned) (ROW == 64 ? ry + lane_v : (ry & ~0xff) | ((ry + lane_v) & 0xf8));
    };
    auto addr_u = [&](int rx) __attribute__((always_inline)) {
        return (unsigned) (ROW == 64 ? rx + lane_u : (rx & ~0xff) | ((rx + lane_u) & 0xfc));
    };
    auto addr_u16 = [&](int rx) __attribute__((always_inline)) {         // whole column tap
        return (unsigned) (ROW == 64 ? rx + lane_u16 : (rx & ~0xff) | ((rx + lane_u16) & 0xf8));
    };
    // pair form: row tap of row block rb, column tap component of column block cb
    auto addr_pv = [&](int ry, int rb) __attribute__((always_inline)) {
        return (unsigned) (ROW == 64 ? ry + lane_pv + 128 * rb : (ry & ~0xff) | ((ry + lane_pv + 128 * rb) & 0xf8));
    };
    auto addr_pu = [&](int rx, int cb) __attribute__((always_inline)) {
        return (unsigned) (ROW == 64 ? rx + lane_pu + 64 * cb : (rx & ~0xff) | ((rx + lane_pu + 64 * cb) & 0xfc));
    };
    // pair form: this lane's operands of one visibility (record r, samples at index idx)
    auto pair_read = [&](const int2 &r, int idx, float2 (&c)[P], v2f (&kv)[2], v2f (&bb)[2])
        __attribute__((always_inline)) {
        if constexpr (ROW == 64 && !TG) {
            // both LDS base addresses with ONE 64-bit add, as in stage_b; the two row taps are one
            // ds_read2_b64, the four column components two ds_read2_b32
            typedef const __attribute__((address_space(3))) v2f *lds_f2;
            typedef const __attribute__((address_space(3))) float *lds_f;
            const uint64_t sum = (((uint64_t) (unsigned) r.y << 32) | (unsigned) r.x) + lane_puv;
            const unsigned au = (unsigned) sum, av = (unsigned) (sum >> 32);
            kv[0] = *reinterpret_cast<lds_f2>((uintptr_t) av);
            kv[1] = *reinterpret_cast<lds_f2>((uintptr_t) (av + 128));            // row + 16
            bb[0].x = *reinterpret_cast<lds_f>((uintptr_t) au);
            bb[0].y = *reinterpret_cast<lds_f>((uintptr_t) (au + 64));            // column + 8
            bb[1].x = *reinterpret_cast<lds_f>((uintptr_t) (au + 128));
            bb[1].y = *reinterpret_cast<lds_f>((uintptr_t) (au + 192));
        } else {
#pragma unroll
            for (int rb = 0; rb < 2; rb++)
                kv[rb] = *reinterpret_cast<const v2f *>(tbytes + addr_pv(r.y, rb));
            bb[0].x = *reinterpret_cast<const float *>(tbytes + addr_pu(r.x, 0));
            bb[0].y = *reinterpret_cast<const float *>(tbytes + addr_pu(r.x, 1));
            bb[1].x = *reinterpret_cast<const float *>(tbytes + addr_pu(r.x, 2));
            bb[1].y = *reinterpret_cast<const float *>(tbytes + addr_pu(r.x, 3));
        }
#pragma unroll
        for (int p = 0; p < P; p++)
            c[p] = *reinterpret_cast<const float2 *>(
                reinterpret_cast<const unsigned char *>(samples + p * 64 + idx) + lane_ps);
    };
    // pair form: the 8 MFMAs of one pair (or of one visibility with a zero partner)
    auto pair_mfma = [&](const float (&a)[P][2], const v2f (&bb)[2]) __attribute__((always_inline)) {
        if constexpr (PAIR)
#pragma unroll
        for (int p = 0; p < P; p++)
#pragma unroll
            for (int rb = 0; rb < 2; rb++)
#pragma unroll
                for (int cb = 0; cb < 4; cb++)
                    acc.t[p][4 * rb + cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                        a[p][rb], (cb & 1) ? bb[cb >> 1].y : bb[cb >> 1].x, acc.t[p][4 * rb + cb], 0, 0, 0);
    };

    // ---- software-pipeline stages over sub-blocks of SUB staged visibilities ---------------
    int2 rec[SUB];
    auto stage_a = [&](int first) __attribute__((always_inline)) {         // record reads
        if constexpr (F16 || PAIR) {
#pragma unroll
            for (int t = 0; t < SUB / 2; t++)
                rec[t] = recs[first + 2 * t + member];      // this lane's member of pair t
        } else {
#pragma unroll
            for (int t = 0; t < SUB; t++)
                rec[t] = recs[first + t];
        }
    };
    auto stage_b = [&](auto &o, int first) __attribute__((always_inline)) {     // sample + kernel-table reads
        if constexpr (PAIR) {
#pragma unroll
            for (int t = 0; t < SUB / 2; t++) {
                float2 c[P];
                pair_read(rec[t], first + 2 * t + member, c, o.kv[t], o.b[t]);
#pragma unroll
                for (int p = 0; p < P; p++)
                    o.c[p][t] = c[p];
            }
        } else if constexpr (F16) {
#pragma unroll
            for (int t = 0; t < SUB / 2; t++) {
                const unsigned au = addr_u16(rec[t].x);
                o.kv[t] = *reinterpret_cast<const uint2 *>(tbytes + addr_v(rec[t].y));
                o.t0[t] = *reinterpret_cast<const uint2 *>(tbytes + au);
                o.t1[t] = *reinterpret_cast<const uint2 *>(ROW == 64 ? tbytes + au + 128
                                                                     : tbytes + (au ^ 128u));
#pragma unroll
                for (int p = 0; p < P; p++)
                    o.c[p][t] = samples[p * 64 + first + 2 * t + member];
            }
        } else {
#pragma unroll
        for (int t = 0; t < SUB; t++) {
            if constexpr (ROW == 64 && !TG) {
                // both LDS addresses with ONE 64-bit add (v_lshl_add_u64): (rx, ry) + (lane_u,
                // lane_v) with the table's LDS base folded into the lane constants; no carry can
                // cross (LDS addresses are far below 2^32)
                typedef const __attribute__((address_space(3))) v2f *lds_f2;
                typedef const __attribute__((address_space(3))) float *lds_f;
                const uint64_t sum = (((uint64_t) (unsigned) rec[t].y << 32) | (unsigned) rec[t].x)
                                     + lane_uv;
                const unsigned au = (unsigned) sum, av = (unsigned) (sum >> 32);
                const v2f kvt = *reinterpret_cast<lds_f2>((uintptr_t) av);
                o.kv[t] = make_float2(kvt.x, kvt.y);
                o.b[t].x = *reinterpret_cast<lds_f>((uintptr_t) au);
                o.b[t].y = *reinterpret_cast<lds_f>((uintptr_t) (au + 128));        // column + 16
            } else {
            const unsigned au = addr_u(rec[t].x);
            o.kv[t] = *reinterpret_cast<const float2 *>(tbytes + addr_v(rec[t].y));
            o.b[t].x = *reinterpret_cast<const float *>(tbytes + au);
            o.b[t].y = *reinterpret_cast<const float *>(                                 // column + 16
                ROW == 64 ? tbytes + au + 128 : tbytes + (au ^ 128u));
            }
#pragma unroll
            for (int p = 0; p < P; p++)
                o.c[p][t] = *reinterpret_cast<const float2 *>(
                    reinterpret_cast<const unsigned char *>(samples + p * 64 + first + t) + lane_s);
        }
        }
    };
    // fp16 form: the 6 k-slots of this lane's visibility (row operand) and of its column taps
    auto join_tap = [&](const uint2 &tp) __attribute__((always_inline)) {        // -> (re, im) in fp32
        // (scalar on purpose: with v_pk_fma_f32 / v_pk_add_f32 here the results were not repeatable)
        v2f r;
        r.x = f16_bits_to_f32(tp.x & 0xffffu) + f16_bits_to_f32(tp.y & 0xffffu);
        r.y = f16_bits_to_f32(tp.x >> 16) + f16_bits_to_f32(tp.y >> 16);
        return r;
    };
    auto row_operand = [&](const float4 &c, v2f kv, bool zero) __attribute__((always_inline)) {
        // (Re, Im)(s conj kv) * S * T = (sx, sy) kv.re + (sy, -sx) kv.im, two lanes of packed math
        float are = fmaf(c.x, kv.x, c.y * kv.y);
        float aim = fmaf(c.z, kv.x, c.w * kv.y);
        if (zero)
            are = aim = 0.0f;
        u32x4 A;
        A[0] = cvt_pk_f16_rtz(are, aim);                            // (re_hi, im_hi)
        const float re_lo = are - f16_bits_to_f32(A[0] & 0xffffu);
        const float im_lo = aim - f16_bits_to_f32(A[0] >> 16);
        A[1] = A[0];
        A[2] = cvt_pk_f16_rtz(re_lo, im_lo);                        // (re_lo, im_lo)
        A[3] = 0;
        return A;
    };
    auto col_operand = [&](const uint2 &tp) __attribute__((always_inline)) {
        u32x4 B;
        B[0] = __builtin_amdgcn_perm(tp.x, tp.x, sel) ^ flip;
        B[1] = __builtin_amdgcn_perm(tp.y, tp.y, sel) ^ flip;
        B[2] = B[0];
        B[3] = 0;
        return B;
    };
    auto stage_c = [&](const auto &o) __attribute__((always_inline)) {
        if constexpr (PAIR) {
            // all operands first, then the MFMAs back to back
            float a[SUB / 2][P][2];
            v2f b[SUB / 2][2];
#pragma unroll
            for (int t = 0; t < SUB / 2; t++) {
#pragma unroll
                for (int j = 0; j < 2; j++)
                    b[t][j] = o.b[t][j] * v2f{pb_sign, pb_sign};       // v_pk_mul_f32
#pragma unroll
                for (int p = 0; p < P; p++)
#pragma unroll
                    for (int rb = 0; rb < 2; rb++)
                        a[t][p][rb] = fmaf(o.c[p][t].x, o.kv[t][rb].x, o.c[p][t].y * o.kv[t][rb].y);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < SUB / 2; t++)
                pair_mfma(a[t], b[t]);
            return;
        } else if constexpr (F16) {
            u32x4 A[P][SUB / 2], B0[SUB / 2], B1[SUB / 2];
#pragma unroll
            for (int t = 0; t < SUB / 2; t++) {
                const v2f kv = join_tap(o.kv[t]);
#pragma unroll
                for (int p = 0; p < P; p++)
                    A[p][t] = row_operand(o.c[p][t], kv, false);
                B0[t] = col_operand(o.t0[t]);
                B1[t] = col_operand(o.t1[t]);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < SUB / 2; t++)
#pragma unroll
                for (int p = 0; p < P; p++) {
                    acc.t0[p] = __builtin_amdgcn_mfma_f32_32x32x16_f16(
                        __builtin_bit_cast(f16x8, A[p][t]), __builtin_bit_cast(f16x8, B0[t]), acc.t0[p], 0, 0, 0);
                    acc.t1[p] = __builtin_amdgcn_mfma_f32_32x32x16_f16(
                        __builtin_bit_cast(f16x8, A[p][t]), __builtin_bit_cast(f16x8, B1[t]), acc.t1[p], 0, 0, 0);
                }
            return;
        } else {
        // all operands first, then the MFMAs back to back (no VALU -> MFMA wait states)
        float a[P][SUB];
        v2f b[SUB];
#pragma unroll
        for (int t = 0; t < SUB; t++) {
            b[t] = o.b[t] * v2f{b_sign, b_sign};        // one v_pk_mul_f32
#pragma unroll
            for (int p = 0; p < P; p++)
                a[p][t] = fmaf(o.c[p][t].x, o.kv[t].x, o.c[p][t].y * o.kv[t].y);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < SUB; t++)
#pragma unroll
            for (int p = 0; p < P; p++) {
                acc.t0[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[p][t], b[t].x, acc.t0[p], 0, 0, 0);
                acc.t1[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[p][t], b[t].y, acc.t1[p], 0, 0, 0);
            }
        }
    };
    // A group whose visibilities do not share one window position (a jump inside the group):
    // rolled loop, window positioned per visibility, operands re-read from LDS.  Rare.
    auto switch_scale = [&](const int (&E_new)[P]) __attribute__((always_inline)) {
        // the accumulators hold sums in units of the old scale: write them out, then go on
        // in the new one
        bool held = false;
#pragma unroll
        for (int p = 0; p < P; p++)
            held |= E_cur[p] != E_NONE;
        if (have && held)
            flush_window<P, F16>(acc, grid, row_stride, pol_stride, Gg, Wu, Wv, Wu, Wv, true, lane,
                            out_scale);
#pragma unroll
        for (int p = 0; p < P; p++)
            if (E_new[p] != E_NONE && E_new[p] != E_WIDE) {
                E_cur[p] = E_new[p];
                out_scale[p] = ldexpf(1.0f / (S_scale * S_scale), E_new[p]);
            }
    };
    // `unscaled` (fp16 form): the group's samples were staged as they are because they spread over
    // too many binades for one scale; every visibility then checks the accumulators' scale itself.
    auto slow_group = [&](int first, bool unscaled) __attribute__((always_inline)) {
        for (int t = 0; t < GROUP; t++) {
            const int idx = first + t;
            const int2 org = origins[idx];
            float2 c[P];
            bool nz = false;
#pragma unroll
            for (int p = 0; p < P; p++) {
                c[p] = *reinterpret_cast<const float2 *>(
                    reinterpret_cast<const unsigned char *>(samples + p * 64 + idx) + lane_s);
                nz |= (c[p].x != 0.0f) | (c[p].y != 0.0f);
            }
            if (!__builtin_amdgcn_readfirstlane((int) nz))
                continue;
            fit_window(__builtin_amdgcn_readfirstlane(org.x), __builtin_amdgcn_readfirstlane(org.x),
                       __builtin_amdgcn_readfirstlane(org.y), __builtin_amdgcn_readfirstlane(org.y));
            const int2 r = recs[idx];
            if constexpr (PAIR) {
                // one visibility, carried by the first member of a pair; the second contributes 0
                float2 cp[P];
                v2f kv[2], bb[2];
                pair_read(r, idx, cp, kv, bb);
                float a[P][2];
#pragma unroll
                for (int j = 0; j < 2; j++)
                    bb[j] = bb[j] * v2f{pb_sign, pb_sign};
#pragma unroll
                for (int p = 0; p < P; p++)
#pragma unroll
                    for (int rb = 0; rb < 2; rb++)
                        a[p][rb] = member ? 0.0f : fmaf(cp[p].x, kv[rb].x, cp[p].y * kv[rb].y);
                pair_mfma(a, bb);
                continue;
            }
            if constexpr (F16) {
                int vis_shift[P];
#pragma unroll
                for (int p = 0; p < P; p++)
                    vis_shift[p] = 0;
                if (unscaled) {
                    int E_new[P];
                    bool change = false;
#pragma unroll
                    for (int p = 0; p < P; p++) {
                        unsigned m = max(__float_as_uint(c[p].x) & 0x7fffffffu,
                                         __float_as_uint(c[p].y) & 0x7fffffffu);
                        m = (unsigned) __builtin_amdgcn_readfirstlane((int) m);
                        if (m >= 0x7f800000u)
                            m = 0;
                        E_new[p] = E_NONE;
                        if (m != 0 && !keeps_scale(sample_exponent(m), E_cur[p], -14)) {
                            E_new[p] = sample_exponent(m);
                            change = true;
                        }
                    }
                    if (change)
                        switch_scale(E_new);     // (fit_window above has already placed the window)
#pragma unroll
                    for (int p = 0; p < P; p++)
                        vis_shift[p] = E_cur[p] != E_NONE ? -E_cur[p] : 0;
                }
                // one visibility, carried by the first member of a pair; the second contributes 0
                const unsigned au16 = addr_u16(r.x);
                const uint2 kvp = *reinterpret_cast<const uint2 *>(tbytes + addr_v(r.y));
                const uint2 tp0 = *reinterpret_cast<const uint2 *>(tbytes + au16);
                const uint2 tp1 = *reinterpret_cast<const uint2 *>(ROW == 64 ? tbytes + au16 + 128
                                                                           : tbytes + (au16 ^ 128u));
                const v2f kvj = join_tap(kvp);
                const u32x4 B0 = col_operand(tp0), B1 = col_operand(tp1);
#pragma unroll
                for (int p = 0; p < P; p++) {
                    float4 cs = samples[p * 64 + idx];
                    cs.x = ldexpf(cs.x, vis_shift[p]);
                    cs.y = ldexpf(cs.y, vis_shift[p]);
                    cs.z = ldexpf(cs.z, vis_shift[p]);
                    cs.w = ldexpf(cs.w, vis_shift[p]);
                    const u32x4 A = row_operand(cs, kvj, member != 0);
                    acc.t0[p] = __builtin_amdgcn_mfma_f32_32x32x16_f16(
                        __builtin_bit_cast(f16x8, A), __builtin_bit_cast(f16x8, B0), acc.t0[p], 0, 0, 0);
                    acc.t1[p] = __builtin_amdgcn_mfma_f32_32x32x16_f16(
                        __builtin_bit_cast(f16x8, A), __builtin_bit_cast(f16x8, B1), acc.t1[p], 0, 0, 0);
                }
                continue;
            }
            if constexpr (!PAIR) {
            const unsigned au = addr_u(r.x);
            const float2 kv = *reinterpret_cast<const float2 *>(tbytes + addr_v(r.y));
            const float b0 = *reinterpret_cast<const float *>(tbytes + au) * b_sign;
            const float b1 = *reinterpret_cast<const float *>(
                ROW == 64 ? tbytes + au + 128 : tbytes + (au ^ 128u)) * b_sign;
#pragma unroll
            for (int p = 0; p < P; p++) {
                const float a = fmaf(c[p].x, kv.x, c[p].y * kv.y);
                acc.t0[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc.t0[p], 0, 0, 0);
                acc.t1[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc.t1[p], 0, 0, 0);
            }
            }
        }
    };

    for (; p0.b < p0.e; p0 = p1, p1 = p2, p2 = next_pos(p2)) {
        const batch_pos &b = p0;
        // ---- stage batch b (lane i <-> visibility b + i) and its per-group bounds ----------
        int gb_u, gb_v;         // per group of 8 lanes: min | max << 16 of the first-tap coordinates
        int gmax_bits[P];       // fp16 form: bits of the group's largest sample | (spread too wide)
        int Evec[P];            // fp16 form: the scale (exponent) this lane's group was staged with,
                                // E_WIDE (staged unscaled) or E_NONE (no sample yet)
        int count = b.e - b.b < 64 ? (int) (b.e - b.b) : 64;    // staged records (fewer once runs are folded)
        {
            const bool ok = coords_ok(b, r0);
            const int u = (short) (r0.uv.x & 0xffff), v = (short) (r0.uv.x >> 16);
            const int su = (short) (r0.uv.y & 0xffff), sv = (short) (r0.uv.y >> 16);
            int mu = u - uv_bias + ts.tu0, mv = v - uv_bias + ts.tv0;
            // row byte offset (a multiple of ROW * 8) + tap byte offset (< 256)
            int2 r;
            r.x = (ok ? (r0.wp * OV + su) * (ROW * 8) : 0) + ((-mu) & 31) * 8 + u_table;
            r.y = (ok ? (r0.wp * OV + sv) * (ROW * 8) : 0) + ((-mv) & 31) * 8;
            bool live = false;
            float2 sp[P];
#pragma unroll
            for (int p = 0; p < P; p++)
                sp[p] = ok ? make_float2(r0.v[p].x * r0.w[p], r0.v[p].y * r0.w[p])
                           : make_float2(0.0f, 0.0f);                       // grid.py:1046
            // ---- fold runs ---------------------------------------------------------------------
            // Consecutive records with equal (u, v, sub_u, sub_v, w_plane) read the same weight cell
            // and apply the same rank-1 matrix conj(kv) (x) conj(ku): their updates add up to ONE
            // update with the sum of their weighted samples.  Lane i heads a run unless lane i - 1
            // holds the same five integers (a record that fails coords_ok never joins a run; runs
            // are cut at the batch's ends).  A batch of heads only -- every batch of a stream that was
            // merged before -- takes the scalar branch around all of it.
            // (FOLD: the float32 forms with one polarization and single table rows in LDS have no
            // register to spare -- with this block they spill or lose a wave per SIMD -- and keep the
            // plain staging)
            constexpr bool FOLD = !(P == 1 && ROW == 32 && !TG && !F16);
            uint64_t heads = ~0ull;
            bool head = true;
            if (FOLD && !(dbg & 4)) {
                const int pux = __builtin_amdgcn_update_dpp(0, r0.uv.x, 0x138, 0xf, 0xf, false);   // wave_shr:1
                const int puy = __builtin_amdgcn_update_dpp(0, r0.uv.y, 0x138, 0xf, 0xf, false);
                const int pwp = __builtin_amdgcn_update_dpp(0, r0.wp, 0x138, 0xf, 0xf, false);
                head = !(lane > 0 && ok && pux == r0.uv.x && puy == r0.uv.y && pwp == r0.wp);
                heads = __ballot(head);
            }
            if (!FOLD || heads == ~0ull) {
                recs[lane] = r;
                origins[lane] = make_int2(mu, mv);
            } else {
                // compact: the heads move up to slots 0 .. count - 1 in order; the slots behind them
                // are staged dead, as the tail of a short batch is (lanes >= count are heads: not ok)
                const uint64_t hv = count == 64 ? heads : heads & ((1ull << count) - 1);
                const int rank = (int) __builtin_amdgcn_mbcnt_hi((unsigned) (hv >> 32),
                                                                 __builtin_amdgcn_mbcnt_lo((unsigned) hv, 0u));
                const bool keep = head && lane < count;
                count = __builtin_popcountll(hv);
                // segmented sum towards the head: after the steps below d, a lane holds the sum of
                // itself and the next d - 1 lanes of its run; `rem` = lanes of the run behind this one
                const uint64_t above = (heads >> lane) >> 1;
                const int rem = above ? __builtin_ctzll(above) : 63 - lane;
#pragma unroll 1
                for (int d = 1; d < 64; d *= 2) {
                    const bool take = d <= rem;
                    if (__ballot(take) == 0)
                        break;                          // (uniform) no run of the batch is that long
#pragma unroll
                    for (int p = 0; p < P; p++) {
                        const float x = __shfl_down(sp[p].x, d, WAVE), y = __shfl_down(sp[p].y, d, WAVE);
                        sp[p].x += take ? x : 0.0f;
                        sp[p].y += take ? y : 0.0f;
                    }
                }
                if (keep) {
                    recs[rank] = r;
                    origins[rank] = make_int2(mu, mv);
#pragma unroll
                    for (int p = 0; p < P; p++)
                        *reinterpret_cast<float2 *>(samples + p * 64 + rank) = sp[p];
                }
                __builtin_amdgcn_wave_barrier();
                // lane j goes on with the record of slot j
                const bool kept = lane < count;
                const int2 org = origins[lane];
                mu = kept ? org.x : mu;
                mv = kept ? org.y : mv;
#pragma unroll
                for (int p = 0; p < P; p++) {
                    const float2 t = *reinterpret_cast<const float2 *>(samples + p * 64 + lane);
                    sp[p] = kept ? t : make_float2(0.0f, 0.0f);
                }
                if (!kept)
                    recs[lane] = make_int2(u_table, 0);
            }
            if constexpr (F16) {
                // keep the samples in fp16 range: a scale T = 2^-E per group of 8 visibilities and
                // polarization (see keeps_scale / T_SPREAD above), chosen group after group so that
                // it changes only when it must
#pragma unroll
                for (int p = 0; p < P; p++) {
                    unsigned m = max(__float_as_uint(sp[p].x) & 0x7fffffffu,
                                     __float_as_uint(sp[p].y) & 0x7fffffffu);
                    if (m >= 0x7f800000u)
                        m = 0;      // NaN / Inf samples poison their own footprint, not the scale
                    const int gmax = group8_max((int) m);
                    const int gmin = group8_min(m ? (int) m : INT_MAX);
                    // low bit of the group maximum := "spread too wide" (the mantissa's last bit
                    // does not matter to the choice of scale)
                    const bool wide = gmax != 0 && (gmax >> 23) - (gmin >> 23) > T_SPREAD;
                    gmax_bits[p] = (gmax & ~1) | (wide ? 1 : 0);
                }
                int Eg[GROUP_COUNT][P];
#pragma unroll
                for (int g = 0; g < GROUP_COUNT; g++) {
#pragma unroll
                    for (int p = 0; p < P; p++) {
                        const unsigned gm = (unsigned) __builtin_amdgcn_readlane(gmax_bits[p], g * GROUP);
                        if ((gm & ~1u) != 0 && !(gm & 1u)
                            && !keeps_scale(sample_exponent(gm), E_stage[p]))
                            E_stage[p] = sample_exponent(gm);
                        Eg[g][p] = E_stage[p];
                    }
                }
                // a group with a wide spread in ANY polarization is staged unscaled in all of them
                bool wide_lane = false;
#pragma unroll
                for (int p = 0; p < P; p++)
                    wide_lane |= (gmax_bits[p] & 1) != 0;
#pragma unroll
                for (int p = 0; p < P; p++) {
                    int e = E_NONE;     // (no sample of this polarization so far: nothing to scale)
#pragma unroll
                    for (int g = 0; g < GROUP_COUNT; g++)
                        e = (lane >> 3) == g ? Eg[g][p] : e;
                    Evec[p] = wide_lane ? E_WIDE : e;
                    const int shift = (wide_lane || e == E_NONE) ? 0 : -e;
                    sp[p].x = ldexpf(sp[p].x, shift);
                    sp[p].y = ldexpf(sp[p].y, shift);
                }
            }
#pragma unroll
            for (int p = 0; p < P; p++) {
                samples[p * 64 + lane] = make_float4(sp[p].x, sp[p].y, sp[p].y, -sp[p].x);
                live |= (sp[p].x != 0.0f) | (sp[p].y != 0.0f);
            }
            // bounds over each aligned group of 8 lanes; dead visibilities do not constrain
            // (first-tap coordinates fit 16 bits: |u| < 32768 and the kernel is at most 64 wide)
            const int gmin_u = group8_min(live ? mu : SHRT_MAX);
            const int gmax_u = group8_max(live ? mu : SHRT_MIN);
            const int gmin_v = group8_min(live ? mv : SHRT_MAX);
            const int gmax_v = group8_max(live ? mv : SHRT_MIN);
            gb_u = (gmax_u << 16) | (gmin_u & 0xffff);
            gb_v = (gmax_v << 16) | (gmin_v & 0xffff);
        }
        // advance the global prefetch pipeline: b+64 gets its (dependent) weight gather,
        // b+128 its raw loads
        r0 = r1;
        if (p1.b < p1.e)
            gather(p1, r0);
        if (p2.b < p2.e)
            load_raw(p2, r1);
        __builtin_amdgcn_wave_barrier();        // LDS is in-order per wave; just pin the order

        const int npairs = (count + 2 * SUB - 1) / (2 * SUB);
        typename std::conditional<F16, pair_ops<P, SUB / 2>,
                                  typename std::conditional<PAIR, pair32_ops<P, SUB / 2>, sub_ops<P, SUB>>::type>::type X, Y;
        stage_a(0);
        stage_b(X, 0);
        stage_a(SUB);
        __builtin_amdgcn_sched_barrier(0);
        // Outer loop: decide how the group starting at pair q is handled (this is where the
        // window moves and cells are flushed).  Inner loop: the hot path, free of any flush
        // code so that the accumulators stay put in their registers; it runs on through the
        // following groups for as long as they fit the current window.
        // (the decision is a plain scalar branch: each arm has its own copy of the pipeline step, so
        // that no loop-carried flag has to live in a vector register)
        auto group_bounds = [&](int first, int &lo_u, int &hi_u, int &lo_v, int &hi_v)
            __attribute__((always_inline)) {
            // (min | max << 16) per axis: two v_readlane instead of four
            const int bu = __builtin_amdgcn_readlane(gb_u, first);
            const int bv = __builtin_amdgcn_readlane(gb_v, first);
            lo_u = (short) (bu & 0xffff);
            hi_u = bu >> 16;
            lo_v = (short) (bv & 0xffff);
            hi_v = bv >> 16;
        };
        auto step = [&](int q, auto live_tag) __attribute__((always_inline)) {
            constexpr bool LIVE = decltype(live_tag)::value;
            const int first = q * 2 * SUB;
            // clamp look-ahead indices at the end of the batch (those operands are unused)
            const int next = q + 1 < npairs ? first + 2 * SUB : first;
            stage_b(Y, first + SUB);
            stage_a(next);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (LIVE)
                stage_c(X);
            __builtin_amdgcn_sched_barrier(0);
            stage_b(X, next);
            stage_a(next + SUB);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (LIVE)
                stage_c(Y);
            __builtin_amdgcn_sched_barrier(0);
        };
        // fp16 form: the scale group `first` was staged with, against the accumulators' scale:
        // 0 = the same (or nothing staged), 1 = another one (flush, then switch), 2 = staged
        // unscaled (one visibility at a time)
        int group_E[P];
        auto group_scale = [&](int first) __attribute__((always_inline)) {
            int verdict = 0;
            if constexpr (F16) {
#pragma unroll
                for (int p = 0; p < P; p++) {
                    group_E[p] = __builtin_amdgcn_readlane(Evec[p], first);
                    if (group_E[p] == E_WIDE)
                        verdict = 2;
                    else if (group_E[p] != E_NONE && group_E[p] != E_cur[p] && verdict == 0)
                        verdict = 1;
                }
            }
            return verdict;
        };
        int q = 0;
        while (q < npairs) {
            int lo_u, hi_u, lo_v, hi_v;
            group_bounds(q * 2 * SUB, lo_u, hi_u, lo_v, hi_v);
            const bool any = lo_u <= hi_u;
            const bool jump = hi_u - lo_u > Su || hi_v - lo_v > Sv;
            const int scale_verdict = any ? group_scale(q * 2 * SUB) : 0;
            if (scale_verdict == 1)
                switch_scale(group_E);
            if (any && !jump && scale_verdict != 2) {
                fit_window(lo_u, hi_u, lo_v, hi_v);     // whole group shares one window
                for (;;) {
                    step(q, std::true_type());
                    q++;
                    if (q >= npairs)
                        break;
                    if ((q * 2 * SUB) % GROUP == 0) {
                        // peek at the next group: stay in the hot loop only if it needs no flush
                        group_bounds(q * 2 * SUB, lo_u, hi_u, lo_v, hi_v);
                        const bool fits = lo_u <= hi_u && lo_u >= Wu && hi_u <= Wu + Su
                                          && lo_v >= Wv && hi_v <= Wv + Sv
                                          && group_scale(q * 2 * SUB) == 0;
                        if (!fits)
                            break;
                    }
                }
            } else {
                if (any)
                    slow_group(q * 2 * SUB, scale_verdict == 2);
                // the group's operands still pass through the pipeline (unused)
                do {
                    step(q, std::false_type());
                    q++;
                } while (q < npairs && (q * 2 * SUB) % GROUP != 0);
            }
        }
        // the next batch overwrites this wave's staging area
        __builtin_amdgcn_wave_barrier();
    }
    if (have && !(dbg & 1))
        flush_window<P, F16>(acc, grid, row_stride, pol_stride, Gg, Wu, Wv, Wu, Wv, true, lane, out_scale);
#ifdef KIMG_GRID_TIMING
    if (g_timing && lane == 0) {
        g_timing[2 * wave_id] = t_begin;
        g_timing[2 * wave_id + 1] = wall_clock64();
    }
#endif
}

// The kernel: the stream as the host gave it, or -- `folded` non-null and its use_folded set -- the one
// the fold pre-pass (grid_fold.hip) compacted from it.  The host cannot know how many records that
// one has, so the division of the stream follows the device's count: the host's plan keeps its
// number of workgroups, the span of a workgroup, the chunk length and the scramble multiplier
// (coprime to the DEVICE's number of chunks) are recomputed here, all of it uniform scalar work.
// DEVICE_COUNT: the instance that a call with the pre-pass launches; calls without it launch the
// other one, which has no prologue: the registers, scratch and occupancy of every such instance are
// those of before the pre-pass existed, and all but five fp16-form instances also spill the same
// number of SGPRs (profiles/prefold_gridder_resources.txt; the prologue's scalars, live through the
// body, cost the other variant 2 to 30 more spilled SGPRs).  The price is twice the instances.
template <int P, int NW, int SUB, int ROW, bool TWO, bool TG, bool F16, bool PAIR, bool DEVICE_COUNT>
__global__ __launch_bounds__(NW * 64) void grid_mfma_kernel(
    float *__restrict__ grid, int64_t row_stride, int64_t pol_stride, int Gg,
    const float *__restrict__ weights_grid, int64_t wg_row_stride, int64_t wg_pol_stride,
    const int16_t *__restrict__ uv, const int16_t *__restrict__ w_plane,
    const float2 *__restrict__ vis, int64_t num_vis,
    const float2 *__restrict__ kern, int W, int OV, tap_split ts, int64_t vis_per_block,
    int p_total, int dbg, const unsigned char *__restrict__ padded,
    const unsigned *__restrict__ tab_max, int64_t chunk, int64_t scramble, unsigned long long *queue,
    const kimg_fold_header *__restrict__ folded)
{
    if (DEVICE_COUNT && folded->use_folded) {
        // (bits 16-17 of dbg: the first polarization of this launch within a record)
        uv = folded->uv;
        w_plane = folded->w_plane;
        vis = folded->vis + ((dbg >> 16) & 3);
        num_vis = folded->count;
        const int64_t waves = (int64_t) gridDim.x * NW;
        vis_per_block = window_vis_per_block_of(num_vis, (int) gridDim.x, NW);
        chunk = window_chunk_of(num_vis, waves, INTERLEAVE_MIN_CHUNK, INTERLEAVE_MAX_PARTS);
        scramble = chunk > 0 ? window_scramble_of((num_vis + chunk - 1) / chunk) : 1;
    }
    grid_mfma_body<P, NW, SUB, ROW, TWO, TG, F16, PAIR>(
        grid, row_stride, pol_stride, Gg, weights_grid, wg_row_stride, wg_pol_stride, uv, w_plane, vis,
        num_vis, kern, W, OV, ts, vis_per_block, p_total, dbg, padded, tab_max, chunk, scramble, queue);
}

// The fp16 form's tables in HBM: pad_table_kernel (kimg_window_launch.h) with the taps scaled by S
// (from the largest |component| of the whole table, *tab_max) and split into fp16 hi/lo pairs, as
// the kernel does in LDS for tables that live there.
template <int ROW>
__global__ __launch_bounds__(256) void pad_table_f16_kernel(
    const float2 *__restrict__ kern, int rows, int K, int tap0, int Kp, float2 *__restrict__ out,
    const unsigned *__restrict__ tab_max)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * ROW)
        return;
    const int row = idx / ROW, t = idx & 31;
    const float2 v = t < Kp ? kern[(int64_t) row * K + tap0 + t] : make_float2(0.0f, 0.0f);
    const unsigned m = *tab_max;
    const int e = (int) (m >> 23) - 127;
    const float S = m ? __uint_as_float((unsigned) (13 - e + 127) << 23) : 1.0f;
    const uint2 split = split_tap(v.x * S, v.y * S);
    out[idx] = make_float2(__uint_as_float(split.x), __uint_as_float(split.y));
}

size_t lds_bytes(int P, int NW, int W, int OV, int row, int tables = 1)
{
    return (size_t) tables * W * OV * row * sizeof(float2)
           + (size_t) NW * 64 * (sizeof(int2) + P * sizeof(float4) + sizeof(int2));
}

// What every launch of one kimg_grid_mfma call over (up to) two polarizations is given
struct grid_call {
    float *g;                       // (the first of these polarizations)
    int64_t row_stride, pol_stride;
    int Gg;
    const float *wg;
    int64_t wg_row_stride, wg_pol_stride;
    const int16_t *uv, *w_plane;
    const float2 *vis;
    int64_t num_vis;
    const float2 *kern;
    int W, OV, p_total;             // (p_total: polarizations per record of the stream)
    hipStream_t stream;
    window_tail tail;
    bool fold;
    const kimg_fold_header *folded; // the fold pre-pass's header, or null: the stream as given
    int p_first;                    // the first of these polarizations within a record
};

template <int P, int ROW, int NW, bool TWO, bool TG, bool F16, bool PAIR, bool DEVICE_COUNT>
int launch_kernel(const grid_call &c, const tap_split &ts);

template <int P, int ROW, int NW, bool TWO, bool TG, bool F16, bool PAIR>
int launch(const grid_call &c, const tap_split &ts)
{
    return c.folded != nullptr ? launch_kernel<P, ROW, NW, TWO, TG, F16, PAIR, true>(c, ts)
                               : launch_kernel<P, ROW, NW, TWO, TG, F16, PAIR, false>(c, ts);
}

template <int P, int ROW, int NW, bool TWO, bool TG, bool F16, bool PAIR, bool DEVICE_COUNT>
int launch_kernel(const grid_call &c, const tap_split &ts)
{
    static_assert(!TWO || TG, "off-diagonal tap blocks read their two tables from HBM");
    constexpr int SUB = (P == 1 && NW <= 12) ? 4 : 2;       // pipeline depth bounded by the VGPR budget
    const size_t lds = TG ? lds_bytes(P, NW, 0, 0, ROW) : lds_bytes(P, NW, c.W, c.OV, ROW);
    const unsigned *tab_max = (TG && F16) ? c.tail.tab_max : nullptr;
    if (TG) {
        const int rows = c.W * c.OV;
        auto pad = [&](int tap0, int Kp, float2 *out) {
            if (F16)
                pad_table_f16_kernel<ROW><<<kimg_divup(rows * ROW, 256), 256, 0, c.stream>>>(
                    c.kern, rows, ts.K, tap0, Kp, out, tab_max);
            else
                pad_table_kernel<ROW><<<kimg_divup(rows * ROW, 256), 256, 0, c.stream>>>(
                    c.kern, rows, ts.K, tap0, Kp, out);
        };
        if (const int rc = window_tables_to_hbm(c.tail, c.kern, rows, ROW, ts, TWO, F16, c.stream, pad))
            return rc;
    }
    if (const int rc = kimg_dynamic_lds(
            reinterpret_cast<const void *>(&grid_mfma_kernel<P, NW, SUB, ROW, TWO, TG, F16, PAIR, DEVICE_COUNT>),
            LDS_LIMIT))
        return rc;
    // bits 8-15: span stagger of a SIMD's waves, percent.  Bits 0-1 (test builds with
    // -DKIMG_NO_ATOMICS, the counterpart of the reference's NO_ATOMICS switch,
    // imager_kernels/atomic.mako:29-40): no end flush / no window flushes -- wrong results, for
    // measuring what the float atomics cost.  Bit 2: runs of records with one sub-cell are NOT folded
    // (KIMG_ARITH_NO_FOLD).  Bits 16-17: the launch's first polarization within a record (for the
    // compacted stream of the fold pre-pass, whose records keep all of them).
#ifdef KIMG_NO_ATOMICS
    const int dbg = (c.p_first << 16) | (12 << 8) | 3 | (c.fold ? 0 : 4);
#else
    const int dbg = (c.p_first << 16) | (12 << 8) | (c.fold ? 0 : 4);
#endif
    // as many blocks resident per CU as the LDS (kernel table + staging) allows.  Long launches:
    // chunks of at least INTERLEAVE_MIN_CHUNK visibilities, up to INTERLEAVE_MAX_PARTS per wave
    const int per_cu = (!TG && lds <= LDS_LIMIT / 2) ? 2 : 1;
    const window_partition part = window_partition_of(
        c.num_vis, NW, kimg_window_cus_now() * per_cu, INTERLEAVE_MIN_CHUNK, INTERLEAVE_MAX_PARTS, true);
    unsigned long long *queue = part.chunk > 0 ? c.tail.queue : nullptr;
    if (queue != nullptr)
        KIMG_HIP(hipMemsetAsync(queue, 0, sizeof(unsigned long long), c.stream));
    grid_mfma_kernel<P, NW, SUB, ROW, TWO, TG, F16, PAIR, DEVICE_COUNT><<<part.blocks, NW * 64, lds, c.stream>>>(
        c.g, c.row_stride, c.pol_stride, c.Gg, c.wg, c.wg_row_stride, c.wg_pol_stride, c.uv, c.w_plane,
        c.vis, c.num_vis, c.kern, c.W, c.OV, ts, part.vis_per_block, c.p_total, dbg, c.tail.padded,
        tab_max, part.chunk, part.scramble, queue, c.folded);
    return kimg_launch_status();
}

// The kernel of a launch, but for its arithmetic form
template <int P_, int ROW_, int NW_, bool TWO_, bool TG_>
struct grid_leaf {
    static constexpr int P = P_, ROW = ROW_, NW = NW_;
    static constexpr bool TWO = TWO_, TG = TG_;
};

// f(grid_leaf) for a launch over pn (1 or 2) polarizations of one tap block; `two`: an off-diagonal
// block, whose two tables are in HBM whatever their size; `in_lds`: where the one table of any other
// block is.
template <class F>
int grid_choose_leaf(int pn, bool two, bool in_lds, int W, int OV, F &&f)
{
    auto fits = [&](int P, int NW, int row) { return lds_bytes(P, NW, W, OV, row) <= LDS_LIMIT; };
    // tables in HBM: doubled rows (5 % faster than single rows), 12-wave blocks (P = 1) as for the
    // LDS form
    if (two)
        return pn == 1 ? f(grid_leaf<1, 64, 12, true, true>{}) : f(grid_leaf<2, 64, 8, true, true>{});
    if (!in_lds)
        return pn == 1 ? f(grid_leaf<1, 64, 12, false, true>{}) : f(grid_leaf<2, 64, 8, false, true>{});
    // table in LDS: doubled rows when they leave room for the staging area, single rows otherwise
    if (pn == 2)
        return fits(2, 8, 64) ? f(grid_leaf<2, 64, 8, false, false>{})
                              : f(grid_leaf<2, 32, 8, false, false>{});
    // 12-wave blocks, one per CU (LDS-bound), when the doubled table leaves room
#ifdef KIMG_GRID_NW16
    if (fits(1, 16, 64))
        return f(grid_leaf<1, 64, 16, false, false>{});
#endif
    if (fits(1, 12, 64))
        return f(grid_leaf<1, 64, 12, false, false>{});
    if (fits(1, 8, 64))
        return f(grid_leaf<1, 64, 8, false, false>{});
    return f(grid_leaf<1, 32, 8, false, false>{});
}

} // namespace

// The kernels are instantiated for 1 and 2 polarizations (32 accumulator registers each keep
// two waves per SIMD without spills); 3 or 4 polarizations run as 2 + 1 / 2 + 2.  Kernel widths
// 33..64 run as 2 x 2 tap blocks: the diagonal blocks like a narrow kernel, with one single-row or
// doubled table in LDS when it fits, the off-diagonal ones with two doubled tables in HBM.  Their
// workspace is sized by whether two single-row tables would fit LDS:
static bool tables_fit_lds(int P, int w_planes, int oversample, int kernel_width)
{
    const int tables = kernel_width > WIN ? 2 : 1;
    return lds_bytes(P > 1 ? 2 : 1, 8, w_planes, oversample, 32, tables) <= LDS_LIMIT;
}

bool kimg_grid_mfma_supported(int P, int w_planes, int oversample, int kernel_width)
{
    // any number of W planes: tables that do not fit LDS are read from a padded copy in HBM
    return P >= 1 && P <= 4 && kernel_width >= 1 && kernel_width <= 2 * WIN
           && (int64_t) w_planes * oversample * 256 * 2 < ((int64_t) 1 << 31);
}

// Where the kernel reads its table from: LDS when it fits -- except for the off-diagonal tap
// blocks of wide kernels, whose two single-row tables in LDS are no faster than doubled rows in
// HBM (the diagonal blocks need one table and always take the LDS form when it fits).
static bool table_in_lds(int P, int w_planes, int oversample, int kernel_width)
{
    return tables_fit_lds(P, w_planes, oversample, kernel_width) && kernel_width <= WIN;
}

// Scratch: the padded table copy (none when the kernel reads its table from LDS) and the tail of
// 256 bytes (window_tail, kimg_window_launch.h).  Between the two, when the caller gave that much
// more, the fold pre-pass's workspace (kimg_grid_prefold_workspace_bytes).
size_t kimg_grid_mfma_workspace_bytes(int P, int w_planes, int oversample, int kernel_width)
{
    if (!kimg_grid_mfma_supported(P, w_planes, oversample, kernel_width))
        return 0;
    const bool fits = tables_fit_lds(P, w_planes, oversample, kernel_width);
    if (fits && kernel_width <= WIN)
        return 256;
    return (size_t) w_planes * oversample * 64 * sizeof(float2) * (kernel_width > WIN ? 2 : 1) + 256;
}

// Below this many records a call does not take the fold pre-pass by itself (KIMG_ARITH_PREFOLD takes
// it at any length).  On a stream without duplicates the count pass buys nothing, and it shows: with
// the bound at 4 Mi the resident store's W-slices (6.85 and 7.25 M merged records) went from 0.681-0.684
// to 0.705-0.716 ms and from 0.725-0.727 to 0.750-0.763 ms per launch (bench.py --full, three runs each
// way), outside their own spread.  Track streams of 1 and 4 Mi records would gain (0.078 -> 0.065,
// 0.250 -> 0.124 ms), but nothing cheap tells the two kinds apart before the count pass has run, so
// the bound lies above the store's slices.  DESIGN 5.1 has the figures.  A caller that has measured
// its stream once needs no bound: it brings a fold plan (kimg_grid_planned) or KIMG_ARITH_NO_PREFOLD.
#ifndef KIMG_PREFOLD_MIN_VIS
#define KIMG_PREFOLD_MIN_VIS (8 << 20)
#endif

size_t kimg_grid_prefold_workspace_bytes(int64_t num_vis, int P)
{
    return kimg_fold_workspace_bytes(P, num_vis / 2);
}

int64_t kimg_grid_prefold_min_vis() { return KIMG_PREFOLD_MIN_VIS; }

int kimg_grid_mfma(void *grid, int64_t grid_row_stride, int64_t grid_pol_stride, int grid_size,
                   int P, const float *weights_grid, int64_t wg_row_stride, int64_t wg_pol_stride,
                   const int16_t *uv, const int16_t *w_plane, const void *vis, int64_t num_vis,
                   const void *convolve_kernel, int w_planes, int oversample, int kernel_width,
                   void *workspace, size_t workspace_bytes, int arith, hipStream_t stream,
                   const void *fold_plan, const void *fold_map)
{
    const bool fold = !(arith & KIMG_ARITH_NO_FOLD);
    const bool prefold_never = (arith & KIMG_ARITH_NO_PREFOLD) != 0;
    // (a fold plan or map is the caller's statement that the stream folds: the pre-pass at any length)
    const bool prefold_always = (arith & KIMG_ARITH_PREFOLD) != 0 || fold_plan != nullptr
                                || fold_map != nullptr;
    arith &= ~(KIMG_ARITH_NO_FOLD | KIMG_ARITH_PREFOLD | KIMG_ARITH_NO_PREFOLD);
    const bool in_lds = table_in_lds(P, w_planes, oversample, kernel_width);
    if (!in_lds && (workspace == nullptr
                    || workspace_bytes < kimg_grid_mfma_workspace_bytes(P, w_planes, oversample,
                                                                       kernel_width)))
        return KIMG_EWORKSPACE;
    const window_tail tail = window_tail_of(workspace, workspace_bytes);
    // The fold pre-pass, once for all the launches below, when the workspace has room for it between
    // the tables and the tail (a workspace of the size before the pre-pass existed, or none: the call
    // goes on without it).  Its kernels read 16 bytes at a time.
    const kimg_fold_header *folded = nullptr;
    const size_t own_bytes = kimg_grid_mfma_workspace_bytes(P, w_planes, oversample, kernel_width);
    auto aligned16 = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    if (fold && !prefold_never && (prefold_always || num_vis >= KIMG_PREFOLD_MIN_VIS)
        && workspace != nullptr
        && workspace_bytes >= own_bytes + kimg_grid_prefold_workspace_bytes(num_vis, P)
        && aligned16(uv) && aligned16(w_plane) && aligned16(vis) && aligned16(workspace)) {
        void *fold_ws = static_cast<unsigned char *>(workspace) + (own_bytes - 256);
        if (const int rc = kimg_fold_launch(uv, w_plane, (const float2 *) vis, num_vis, P, num_vis / 2,
                                            fold_ws, stream,
                                            static_cast<const kimg_fold_plan_data *>(fold_plan),
                                            static_cast<const kimg_fold_map_data *>(fold_map)))
            return rc;
        folded = static_cast<const kimg_fold_header *>(fold_ws);
    }
    for (int p0 = 0; p0 < P; p0 += 2) {
        const int pn = P - p0 >= 2 ? 2 : 1;
        const grid_call c = {
            (float *) grid + 2 * p0 * grid_pol_stride, grid_row_stride, grid_pol_stride, grid_size,
            weights_grid + p0 * wg_pol_stride, wg_row_stride, wg_pol_stride, uv, w_plane,
            (const float2 *) vis + p0, num_vis, (const float2 *) convolve_kernel, w_planes,
            oversample, P, stream, tail, fold, folded, p0};
        // The one table of a wide kernel's diagonal blocks fits LDS whenever a narrow kernel's
        // would, by the budget of this launch's polarizations.
        const bool one_in_lds = kernel_width > WIN
            ? lds_bytes(pn, 8, w_planes, oversample, 32) <= LDS_LIMIT : in_lds;
        const int rc = kimg_for_tap_blocks(kernel_width, [&](const tap_split &ts, bool two) {
            return grid_choose_leaf(pn, two, one_in_lds, w_planes, oversample, [&](auto leaf) {
                using L = decltype(leaf);
                // <..., F16, PAIR>: the fp16 hi/lo form or the float32 pair form (two visibilities
                // per matrix instruction), else the exact-fp32 instruction of KIMG_ARITH_FP32_32X32
                if (arith == KIMG_ARITH_SPLIT_FP16)
                    return launch<L::P, L::ROW, L::NW, L::TWO, L::TG, true, false>(c, ts);
                if (arith == KIMG_ARITH_FP32)
                    return launch<L::P, L::ROW, L::NW, L::TWO, L::TG, false, true>(c, ts);
                return launch<L::P, L::ROW, L::NW, L::TWO, L::TG, false, false>(c, ts);
            });
        });
        if (rc)
            return rc;
    }
    return 0;
}

#ifdef KIMG_GRID_TIMING
extern "C" int kimg_debug_grid_timing(void *buffer)
{
    long long *p = static_cast<long long *>(buffer);
    return hipMemcpyToSymbol(HIP_SYMBOL(g_timing), &p, sizeof(p)) == hipSuccess ? 0 : -1;
}
#endif

// (kimg_preload, api.hip)
KIMG_PRELOAD_THIS_UNIT(pad_table_kernel<64>)
