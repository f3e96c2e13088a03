// How a window kernel's launch divides a stream of num_vis records, as functions of the record
// count that the host (window_partition_of, kimg_window_launch.h) and the device (the prologue of
// grid_mfma_kernel, when the fold pre-pass has shortened the stream) evaluate alike; and the window's
// geometry as a function of the kernel width.  Nothing here needs the HIP runtime: the host test of
// these helpers compiles this file alone.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define KIMG_HD __host__ __device__
#else
#define KIMG_HD
#endif

// The window and what a K-tap kernel leaves of it.  The launches (kimg_for_tap_blocks,
// kimg_window_launch.h), the strips of the resident store (store.hip) and the bins of the tile-binned
// variant (grid_binned.hip) all take it from here: an order laid out for another slack than the
// kernels' is an order the window does not follow.
constexpr int WIN = 32;                         // the window: 32 x 32 grid points

// Taps of one launch along one axis: K itself up to 32 taps, (K + 1) / 2-tap blocks above
KIMG_HD inline int window_taps_of(int K) { return K > WIN ? (K + 1) / 2 : K; }

// Cells a footprint origin may move without the window moving
KIMG_HD inline int window_slack(int K) { return WIN - window_taps_of(K); }

// Records per workgroup when every workgroup streams one contiguous span: a multiple of 64, at
// least one batch per wave.  `blocks` workgroups of that span cover the stream.
KIMG_HD inline int64_t window_vis_per_block_of(int64_t num_vis, int blocks, int NW)
{
    int64_t per = (num_vis + blocks - 1) / blocks;
    per = (per + 63) / 64 * 64;
    return per < 64 * NW ? 64 * NW : per;
}

// Chunk length of a launch of `waves` waves that works by the chunk (a multiple of 64), or 0: the
// stream is too short for two chunks of at least min_chunk records per wave.  A wave gets up to
// max_parts chunks.
KIMG_HD inline int64_t window_chunk_of(int64_t num_vis, int64_t waves, int64_t min_chunk,
                                       int64_t max_parts)
{
    int64_t parts = num_vis / (waves * min_chunk);
    parts = parts > max_parts ? max_parts : parts;
    if (parts < 2)
        return 0;
    return ((num_vis + waves * parts - 1) / (waves * parts) + 63) / 64 * 64;
}

// The candidates for the multiplier that scrambles chunk numbers: primes, so that one of them is
// coprime to `chunks` exactly when it does not divide it.  Their product exceeds 2^63: no count
// is divisible by all of them.
constexpr int KIMG_SCRAMBLE_CANDIDATES = 7;
KIMG_HD inline int64_t window_scramble_candidate(int i)
{
    switch (i) {
    case 0: return 7919;
    case 1: return 7907;
    case 2: return 7901;
    case 3: return 7883;
    case 4: return 7879;
    case 5: return 7877;
    default: return 7873;
    }
}

// Ticket t of a launch is chunk (t * m) mod chunks: m must be coprime to the number of chunks OF THE
// STREAM THE KERNEL GRIDS, or tickets skip some chunks and repeat others.
KIMG_HD inline int64_t window_scramble_of(int64_t chunks)
{
    for (int i = 0; i < KIMG_SCRAMBLE_CANDIDATES; i++) {
        const int64_t m = window_scramble_candidate(i);
        if (chunks % m != 0)
            return m;
    }
    return 1;
}
