// Host side of the float32 window kernels (grid_mfma.hip, degrid_mfma.hip): what a launch of either
// needs besides its kernel -- the tap blocks of a call, the workspace's tail, the partition of the
// stream over blocks and chunks, and the tables' padded copy in HBM.  Which kernel a launch runs
// is each file's own business (grid_leaf / degrid_leaf there).
#pragma once
#include "kimg_common.h"
#include "kimg_window_plan.h"

// Private to the including unit, like the kernels it serves (tap_split is a kernel parameter).
namespace {

constexpr size_t LDS_LIMIT = 160 * 1024;        // LDS a workgroup may have on gfx950

// Kernel widths above 32 are (de)gridded as 2 x 2 blocks of taps, one launch per block: the
// launch handles row taps [tv0, tv0 + Kv) and column taps [tu0, tu0 + Ku) of the K-tap kernel
// (each at most 32 wide), which is itself a (de)gridding with a narrower kernel and a shifted
// origin.  Off-diagonal blocks need different row and column taps, hence TWO tables.
struct tap_split {
    int K;              // full kernel width (row stride of the table in HBM, uv_bias)
    int tv0, Kv;        // row (v) taps of this launch
    int tu0, Ku;        // column (u) taps of this launch
};

// f(ts, two) for the one tap block of a kernel of up to 32 taps, or the four of a wider one (row
// block, then column block); `two`: an off-diagonal block.  Diagonal blocks take row and column
// taps from the same half of the table: one table, like a narrow kernel's.  Stops at, and
// returns, the first non-zero result of f.
template <class F> inline int kimg_for_tap_blocks(int K, F &&f)
{
    const bool wide = K > WIN;
    const int Kh = window_taps_of(K);                   // taps per block along one axis
    const int nblk = wide ? 2 : 1;
    for (int jb = 0; jb < nblk; jb++)
        for (int kb = 0; kb < nblk; kb++) {
            const tap_split ts = {K, jb * Kh, jb ? K - Kh : Kh, kb * Kh, kb ? K - Kh : Kh};
            if (const int rc = f(ts, jb != kb))
                return rc;
        }
    return 0;
}

// A window kernel's workspace: the padded copy of tables that do not fit LDS at its start, and a
// tail of 256 bytes -- at workspace_bytes - 256 the table's largest |component| (fp16 form with
// the table in HBM), at workspace_bytes - 128 the chunk counter of long launches.  A caller whose
// tables are in LDS may give less than 256 bytes, or nothing: there is then no maximum to keep,
// and the waves of a long launch take their chunks in a fixed order.
struct window_tail {
    unsigned char *padded;
    unsigned *tab_max;
    unsigned long long *queue;
};

inline window_tail window_tail_of(void *workspace, size_t workspace_bytes)
{
    unsigned char *base = static_cast<unsigned char *>(workspace);
    if (base == nullptr || workspace_bytes < 256)
        return {base, nullptr, nullptr};
    return {base, reinterpret_cast<unsigned *>(base + workspace_bytes - 256),
            reinterpret_cast<unsigned long long *>(base + workspace_bytes - 128)};
}

// How a launch divides its stream.  Every block streams a contiguous span of vis_per_block
// records (a multiple of 64, at least one batch per wave), as many blocks as fill blocks_max.
// Long launches work by the chunk instead (chunk > 0; batch_pos in the kernels): every wave takes
// its work from up to max_parts places of the stream, in chunks of at least min_chunk records.
// (The formulas are kimg_window_plan.h's: the gridder's kernel evaluates them again for a stream
// whose length only the device knows.)
struct window_partition {
    int blocks;
    int64_t vis_per_block, chunk, scramble;
};

inline window_partition window_partition_of(int64_t num_vis, int NW, int blocks_max,
                                            int64_t min_chunk, int64_t max_parts, bool want_scramble)
{
    window_partition p;
    p.vis_per_block = window_vis_per_block_of(num_vis, blocks_max, NW);
    p.blocks = (int) ((num_vis + p.vis_per_block - 1) / p.vis_per_block);
    const int64_t waves = (int64_t) p.blocks * NW;
    p.chunk = window_chunk_of(num_vis, waves, min_chunk, max_parts);
    // (gridder) chunk numbers are scrambled by a multiplier coprime to their count
    p.scramble = 1;
    if (want_scramble && p.chunk > 0)
        p.scramble = window_scramble_of((num_vis + p.chunk - 1) / p.chunk);
    return p;
}

// Zero-padded copy of taps [tap0, tap0 + Kp) of every table row: [rows][ROW] float2 (ROW = 64:
// the 32 taps twice).
template <int ROW>
__global__ __launch_bounds__(256) void pad_table_kernel(
    const float2 *__restrict__ kern, int rows, int K, int tap0, int Kp, float2 *__restrict__ out)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * ROW)
        return;
    const int row = idx / ROW, t = idx & 31;
    out[idx] = t < Kp ? kern[(int64_t) row * K + tap0 + t] : make_float2(0.0f, 0.0f);
}

// The table(s) of a launch that reads them from HBM, into the workspace: row taps first, column
// taps (`two`) behind them, each [rows][row_taps]; before that the table's maximum, where the
// form wants it.  pad(tap0, Kp, out) launches the unit's pad kernel.
template <class Pad>
inline int window_tables_to_hbm(const window_tail &tail, const float2 *kern, int rows, int row_taps,
                                const tap_split &ts, bool two, bool want_max, hipStream_t stream,
                                Pad &&pad)
{
    float2 *out = reinterpret_cast<float2 *>(tail.padded);
    if (want_max)
        if (const int rc = kimg_table_max(reinterpret_cast<const float *>(kern),
                                          (int64_t) rows * ts.K * 2, tail.tab_max, stream))
            return rc;
    pad(ts.tv0, ts.Kv, out);
    if (two)
        pad(ts.tu0, ts.Ku, out + (size_t) rows * row_taps);
    return 0;
}

} // namespace
