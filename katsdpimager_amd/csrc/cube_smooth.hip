// Cube smoothing to a common beam (include/kimg.h, "Cube smoothing to a common beam"): every filled
// plane of a cube [C][P][H][W] convolved with its own small kernel of (2 R_c + 1)^2 taps, R_c <= 16,
// into a second cube, all channels and polarizations in one launch.  katsdpimager_amd/smooth.py holds
// the same contract as numpy (cube_smooth_host) and makes the taps (kernel_tables).
//
// A workgroup of 256 threads makes a tile of 64 x 64 outputs of one plane; thread (tx, ty) of 16 x 16
// makes the 4 x 4 outputs at (4 ty, 4 tx).  The tile and its halo -- 64 + 2 R rows, and 64 + 2 Rup
// columns from x0 - Rup on, Rup = R rounded up to 4 so that every 16-byte load is aligned -- are staged
// in LDS once, zeros beyond the plane, rows CS_STRIDE = 96 floats apart: 36880 bytes whatever R is,
// four workgroups a CU.  A thread then walks its input rows in ascending order and each row in
// 16-byte chunks, two of which are in registers at a time: one ds_read_b128 feeds up to 4 columns of
// taps x 4 output rows x 4 outputs = 64 products.  Per output the products are added in the order of
// the contract (dy ascending, then dx ascending), each rounded, nothing fused (the build has
// -ffp-contract=off); the zeros of the border are multiplied and added like any sample, so the bits
// are the twin's.  The taps of the workgroup's channel are read at addresses that are the same for
// every lane (scalar loads); which taps a step has is decided by uniform branches.
// Bank conflicts: the lanes of a wave are 16 tx x 4 ty; a ds_read_b128 is served in groups of 16 lanes
// that take 8 lanes of one ty and 4 + 4 of the next (lanes 0-3, 12-15, 20-27, ...).  The 8 lanes
// cover dwords 16 .. 47 of their row's 64, the 4 + 4 dwords 0 .. 15 and 48 .. 63 of theirs, and the
// two rows are 4 * 96 = 384 = 6 * 64 dwords apart: the same bank row, no bank twice.
// A channel that is not filled returns at once; one with R = 0 is a scaled copy without LDS.
#include "kimg_cube_column.h"

namespace {

constexpr int CS_MAX_R = KIMG_CUBE_SMOOTH_MAX_RADIUS;
constexpr int CS_TILE = 64;                     // outputs of a workgroup, each way
constexpr int CS_THREADS = 256;
constexpr int CS_STRIDE = CS_TILE + 2 * CS_MAX_R;      // floats between rows of the LDS tile
constexpr int CS_ROWS = CS_TILE + 2 * CS_MAX_R;
// (the last chunk a thread loads, never one it uses, may lie 4 floats past the last row)
constexpr int CS_LDS_FLOATS = CS_ROWS * CS_STRIDE + 4;
constexpr unsigned CS_NOT_FILLED = 31;

// The radius of every channel, or CS_NOT_FILLED, 5 bits each and 6 to a word, a kernel argument BY
// VALUE: the same for every lane, read through the scalar path; no table in device memory.
struct cs_radii {
    uint32_t w[(COL_MAX_CHANNELS + 5) / 6];
};

inline void cs_set(cs_radii &r, int c, unsigned code) { r.w[c / 6] |= code << (5 * (c % 6)); }

__device__ inline int cs_get(const cs_radii &r, int c) { return (r.w[c / 6] >> (5 * (c % 6))) & 31u; }

// V = 4: 16-byte loads and stores (base, pitches and W multiples of 4 floats); V = 1: one pixel each
template <int V>
__global__ __launch_bounds__(CS_THREADS)
void cube_smooth_kernel(const float *__restrict__ cube, int64_t pitch, float *__restrict__ out,
                        int64_t out_pitch, int H, int W, int tiles_x, const cs_radii radii,
                        const float *__restrict__ taps, int64_t taps_pitch)
{
    __shared__ __attribute__((aligned(16))) float tile[CS_LDS_FLOATS];
    const int c = blockIdx.z;
    const int R = cs_get(radii, c);
    if (R > CS_MAX_R)
        return;
    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int x0t = tile_x * CS_TILE, y0t = tile_y * CS_TILE;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int x0 = x0t + 4 * tx, y0 = y0t + 4 * ty;
    const int64_t plane = (int64_t) blockIdx.y * H * W;
    const float *src = cube + (int64_t) c * pitch + plane;
    float *dst = out + (int64_t) c * out_pitch + plane;
    const float *k = taps + (int64_t) c * taps_pitch;

    float acc[4][4];
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int i = 0; i < 4; i++)
            acc[j][i] = 0.0f;

    if (R == 0) {
        const float tap = k[0];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int y = y0 + j;
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (y < H) {
                const float *p = src + (int64_t) y * W + x0;
                if constexpr (V == 4) {
                    if (x0 < W)
                        col_load<4>(p, v);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        if (x0 + i < W)
                            v[i] = p[i];
                }
            }
#pragma unroll
            for (int i = 0; i < 4; i++)
                acc[j][i] = acc[j][i] + tap * v[i];
        }
    } else {
        const int Rup = (R + 3) & ~3;
        const int rows = CS_TILE + 2 * R;
        const int xa = x0t - Rup, ya = y0t - R;         // what LDS (0, 0) holds
        if constexpr (V == 4) {
            const int quads = (CS_TILE + 2 * Rup) / 4;
            for (int n = threadIdx.x; n < rows * quads; n += CS_THREADS) {
                const int row = n / quads, q = n - row * quads;
                const int y = ya + row, x = xa + 4 * q;
                // (x and W are multiples of 4: a quad is inside the plane or outside it)
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (y >= 0 && y < H && x >= 0 && x < W)
                    v = *reinterpret_cast<const float4 *>(src + (int64_t) y * W + x);
                *reinterpret_cast<float4 *>(tile + row * CS_STRIDE + 4 * q) = v;
            }
        } else {
            const int cols = CS_TILE + 2 * Rup;
            for (int n = threadIdx.x; n < rows * cols; n += CS_THREADS) {
                const int row = n / cols, col = n - row * cols;
                const int y = ya + row, x = xa + col;
                float v = 0.0f;
                if (y >= 0 && y < H && x >= 0 && x < W)
                    v = src[(int64_t) y * W + x];
                tile[row * CS_STRIDE + col] = v;
            }
        }
        __syncthreads();

        // Output (y0 + j, x0 + i), tap (dy, dx): LDS row 4 ty + rr with rr = dy + R + j, LDS column
        // 4 tx + s + i with s = dx + R + (Rup - R), the step of the row walk
        const int D = 2 * R + 1;
        const int first = Rup - R;
        const int groups = (first + D + 3) >> 2;
        for (int rr = 0; rr < D + 3; rr++) {
            const float *row = tile + (4 * ty + rr) * CS_STRIDE + 4 * tx;
            float4 prev = *reinterpret_cast<const float4 *>(row);
            for (int g = 0; g < groups; g++) {
                const float4 cur = *reinterpret_cast<const float4 *>(row + 4 * g + 4);
                const float w[8] = {prev.x, prev.y, prev.z, prev.w, cur.x, cur.y, cur.z, cur.w};
#pragma unroll
                for (int m = 0; m < 4; m++) {
                    const int t = 4 * g + m - first;            // dx + R
                    if (t < 0 || t >= D)
                        continue;
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const int u = rr - j;                   // dy + R
                        if (u < 0 || u >= D)
                            continue;
                        const float tap = k[u * D + t];
#pragma unroll
                        for (int i = 0; i < 4; i++)
                            acc[j][i] = acc[j][i] + tap * w[m + i];
                    }
                }
                prev = cur;
            }
        }
    }

#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int y = y0 + j;
        if (y >= H)
            continue;
        float o[4];
#pragma unroll
        for (int i = 0; i < 4; i++)
            o[i] = acc[j][i] != acc[j][i] ? col_nan() : acc[j][i];
        float *p = dst + (int64_t) y * W + x0;
        if constexpr (V == 4) {
            if (x0 < W)
                col_store<4>(p, o);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (x0 + i < W)
                    p[i] = o[i];
        }
    }
}

}  // namespace

extern "C" int kimg_cube_smooth(const float *cube, int64_t channel_pitch, float *out,
                                int64_t out_channel_pitch, int num_channels, int num_polarizations,
                                int height, int width, const uint8_t *filled_host,
                                const int32_t *radius_host, const float *taps, int64_t taps_pitch,
                                void *stream)
{
    KIMG_CHECK_ARG(cube && out && filled_host && radius_host && taps);
    KIMG_CHECK_ARG(num_channels >= 1 && num_channels <= COL_MAX_CHANNELS);
    KIMG_CHECK_ARG(num_polarizations >= 1 && height >= 1 && width >= 1);
    KIMG_CHECK_ARG(((uintptr_t) cube & 3) == 0 && ((uintptr_t) out & 3) == 0
                   && ((uintptr_t) taps & 3) == 0);
    // (a channel, the extents in bytes below and every index the kernel forms stay inside int64)
    const int64_t pixels = (int64_t) height * width;
    KIMG_CHECK_ARG(num_polarizations <= INT64_MAX / 8 / pixels);
    const int64_t M = num_polarizations * pixels;
    const int64_t longest = (INT64_MAX / (int64_t) sizeof(float) - M) / num_channels;
    KIMG_CHECK_ARG(channel_pitch >= M && out_channel_pitch >= M);
    KIMG_CHECK_ARG(channel_pitch <= longest && out_channel_pitch <= longest);
    cs_radii radii = {};
    bool any = false;
    for (int c = 0; c < num_channels; c++) {
        if (!filled_host[c]) {
            cs_set(radii, c, CS_NOT_FILLED);
            continue;
        }
        const int R = radius_host[c];
        KIMG_CHECK_ARG(R >= 0 && R <= CS_MAX_R);
        KIMG_CHECK_ARG(taps_pitch >= (int64_t) (2 * R + 1) * (2 * R + 1));
        cs_set(radii, c, (unsigned) R);
        any = true;
    }
    // two cubes that share no byte
    const uintptr_t from = (uintptr_t) cube, to = (uintptr_t) out;
    const uintptr_t from_bytes = ((uintptr_t) (num_channels - 1) * channel_pitch + M) * sizeof(float);
    const uintptr_t to_bytes = ((uintptr_t) (num_channels - 1) * out_channel_pitch + M) * sizeof(float);
    KIMG_CHECK_ARG(from_bytes <= UINTPTR_MAX - from && to_bytes <= UINTPTR_MAX - to);
    KIMG_CHECK_ARG(from + from_bytes <= to || to + to_bytes <= from);
    const int tiles_x = kimg_divup(width, CS_TILE);
    const int64_t tiles = (int64_t) tiles_x * kimg_divup(height, CS_TILE);
    if (tiles > 0x7fffffff || num_polarizations > 65535)
        return KIMG_EUNSUPPORTED;
    if (!any)
        return 0;

    const uintptr_t alignment = from | to | ((uintptr_t) channel_pitch * sizeof(float))
                                | ((uintptr_t) out_channel_pitch * sizeof(float))
                                | ((uintptr_t) width * sizeof(float));
    const dim3 grid((unsigned) tiles, (unsigned) num_polarizations, (unsigned) num_channels);
    hipStream_t s = (hipStream_t) stream;
    if ((alignment & 15) == 0)
        cube_smooth_kernel<4><<<grid, CS_THREADS, 0, s>>>(cube, channel_pitch, out, out_channel_pitch,
                                                          height, width, tiles_x, radii, taps, taps_pitch);
    else
        cube_smooth_kernel<1><<<grid, CS_THREADS, 0, s>>>(cube, channel_pitch, out, out_channel_pitch,
                                                          height, width, tiles_x, radii, taps, taps_pitch);
    return kimg_launch_status();
}

KIMG_PRELOAD_THIS_UNIT((cube_smooth_kernel<1>))
