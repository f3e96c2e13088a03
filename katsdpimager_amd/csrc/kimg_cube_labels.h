// What the units that walk a label cube share (cube_link.hip, cube_sources.hip): the geometry of the
// dense launches -- a workgroup of LK_THREADS threads owns LK_CHUNK consecutive elements of ONE
// channel's plane, a thread LK_V consecutive ones -- the load of a thread's labels, the per-channel
// filled bits and the host's checks of alignment and of the int32 range of the labels.  Everything
// here is local to the including translation unit.
#pragma once
#include "kimg_cube_column.h"

namespace {

constexpr int LK_THREADS = 256;
constexpr int LK_V = 4;
constexpr int LK_CHUNK = LK_THREADS * LK_V;

__device__ inline bool lk_filled(const col_mask &filled, int c)
{
    return (filled.bits[c >> 5] >> (c & 31)) & 1;
}

__device__ inline void lk_label_load(const int32_t *p, int n, int wide, int32_t (&v)[LK_V])
{
    if (wide && n == LK_V) {
        const int4 t = *reinterpret_cast<const int4 *>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int e = 0; e < LK_V; e++)
            v[e] = e < n ? p[e] : 0;
    }
}

col_mask lk_filled_mask(const uint8_t *filled_host, int num_channels)
{
    col_mask filled = {};
    for (int c = 0; c < num_channels; c++)
        if (filled_host[c])
            col_set(filled, c);
    return filled;
}

bool lk_aligned(const void *p, uintptr_t to) { return ((uintptr_t) p & (to - 1)) == 0; }

// C * M fits the labels
bool lk_fits(int num_channels, int64_t plane_elements)
{
    return num_channels <= COL_MAX_CHANNELS && plane_elements <= ((int64_t) INT32_MAX - 1) / num_channels;
}

int64_t lk_blocks_per_channel(int64_t plane_elements) { return (plane_elements + LK_CHUNK - 1) / LK_CHUNK; }

}  // namespace
