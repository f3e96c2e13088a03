// What the units that re-order and compact the record stream share (preprocess.hip, store.hip,
// grid_binned.hip, grid_fold.hip): the workspace carver, the bits of a radix sort, the (key, index)
// sort, and the copy of one record.  A record is uv as int16[4] (read as one int2), w_plane as int16,
// weights as float[P] and vis as float2[P].  Only what at least two of the units use is here;
// everything is local to the including translation unit.  (The window's geometry, which store.hip and
// grid_binned.hip order their streams by, is kimg_window_plan.h's.  The three tests for "two records
// have the same coordinates" stay with their units: DESIGN 5.24.)
#pragma once
#include "kimg_common.h"
#include <hipcub/hipcub.hpp>

namespace {

// A workspace handed out in 256-byte-aligned pieces, in the order they are asked for.  Built on a
// null base it hands out null pointers and only adds up: one carving function per unit serves the
// size query and the call.
struct ws_carver {
    explicit ws_carver(void *workspace) : base(static_cast<unsigned char *>(workspace)) {}
    template <class T> T *take(size_t count)
    {
        unsigned char *p = base ? base + off : nullptr;
        off += (count * sizeof(T) + 255) / 256 * 256;
        return reinterpret_cast<T *>(p);
    }
    size_t total() const { return off; }

    unsigned char *base;
    size_t off = 0;
};

// Low bits that hold every key in 0 .. max_key, never less than 1: the end_bit of a radix sort
inline int sort_bits(unsigned max_key)
{
    int bits = 1;
    while (bits < 32 && (max_key >> bits) != 0)
        bits++;
    return bits;
}

// The stable sort of (key, record number) pairs: a key kernel of the unit fills keys[0] and
// index[0], sort() orders them by the keys' low `bits` bits and hands back the record numbers in
// sorted order (in whichever of the two index buffers the last pass left them).
template <class Key>
struct index_sort {
    Key *keys[2];
    unsigned *index[2];

    // (keys and indices alternate: the order these workspaces have always had)
    void carve(ws_carver &c, int64_t n)
    {
        for (int i = 0; i < 2; i++) {
            keys[i] = c.take<Key>((size_t) n);
            index[i] = c.take<unsigned>((size_t) n);
        }
    }

    // hipCUB's temporary storage for n pairs, sorted on all bits of the key
    static hipError_t temp_bytes(int64_t n, size_t &bytes)
    {
        hipcub::DoubleBuffer<Key> k(nullptr, nullptr);
        hipcub::DoubleBuffer<unsigned> v(nullptr, nullptr);
        bytes = 0;
        return hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, k, v, (int) n, 0,
                                                  (int) (8 * sizeof(Key)), (hipStream_t) 0);
    }

    hipError_t sort(void *temp, size_t temp_size, int64_t n, int bits, hipStream_t stream,
                    const unsigned *&sorted) const
    {
        hipcub::DoubleBuffer<Key> k(keys[0], keys[1]);
        hipcub::DoubleBuffer<unsigned> v(index[0], index[1]);
        const hipError_t e = hipcub::DeviceRadixSort::SortPairs(temp, temp_size, k, v, (int) n, 0,
                                                                bits, stream);
        sorted = v.Current();
        return e;
    }
};

// Record `src` of a stream to place `dst` of another: its coordinates, then its P samples (and,
// with WEIGHTS, its P weights; without, neither `weights` nor `w_out` is touched).  A merge writes
// the two halves itself: the coordinates of a run's first record, the sums it holds.
__device__ __forceinline__ void copy_coords(int64_t dst, int64_t src, const int2 *uv,
                                            const int16_t *w_plane, int2 *uv_out, int16_t *wp_out)
{
    uv_out[dst] = uv[src];
    wp_out[dst] = w_plane[src];
}

template <int P, bool WEIGHTS>
__device__ __forceinline__ void copy_samples(int64_t dst, int64_t src, const float *weights,
                                             const float2 *vis, float *w_out, float2 *vis_out)
{
#pragma unroll
    for (int p = 0; p < P; p++) {
        if (WEIGHTS)
            w_out[dst * P + p] = weights[src * P + p];
        vis_out[dst * P + p] = vis[src * P + p];
    }
}

template <int P, bool WEIGHTS>
__device__ __forceinline__ void copy_record(int64_t dst, int64_t src, const int2 *uv,
                                            const int16_t *w_plane, const float *weights,
                                            const float2 *vis, int2 *uv_out, int16_t *wp_out,
                                            float *w_out, float2 *vis_out)
{
    copy_coords(dst, src, uv, w_plane, uv_out, wp_out);
    copy_samples<P, WEIGHTS>(dst, src, weights, vis, w_out, vis_out);
}

} // namespace
