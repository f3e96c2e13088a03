// Multi-scale CLEAN (include/kimg.h, "Multi-scale CLEAN"): a separable convolution, the set-up of
// the scale residuals and cross patches, and a device-resident minor cycle over several Gaussian
// scales.  An operator of its own next to the Hogbom kernels of clean.hip: it shares their tile
// structure (32 x 32 tiles offset by the border, first strict maximum in row-major order within a
// tile, first maximal tile in row-major tile order) and their arithmetic (every multiply and every
// add rounded on its own: this file is built with -ffp-contract=off and uses no fmaf), so that
// with the single scale 0 it takes the components the Hogbom loop takes, bit for bit.
#include "kimg_common.h"
#include "kimg_peak_key.h"
#include <string.h>

namespace {

constexpr int TILE = 32;
constexpr int MAX_SCALES = KIMG_CLEAN_SCALES_MAX;
constexpr int MAX_RADIUS = KIMG_CLEAN_SCALES_MAX_RADIUS;
constexpr int MAX_PAIRS = MAX_SCALES * (MAX_SCALES + 1) / 2;
constexpr int TAPS_PITCH = 192;         // floats per scale in the tap tables (2 * 64 + 1 used)
constexpr int CROSS_PITCH = 320;        // floats per pair of scales (4 * 64 + 1 used)
constexpr int CHUNK = 64;               // minor cycles enqueued between two looks at `done`

// ---- separable convolution ------------------------------------------------------------------
// out[c] = sum over i = 0 .. 2R of taps[i] * in[c - R + i], in index order from 0.0f, taps that fall
// outside the image skipped.  The kernels take radii up to 2 * MAX_RADIUS: the cross taps of two
// scales have the sum of their radii.
constexpr int CONV_MAX_RADIUS = 2 * MAX_RADIUS;
constexpr int CONV_ROW = 256;           // outputs of a workgroup of the horizontal pass
constexpr int CONV_STRIP = 64;          // columns of a workgroup of the vertical pass
constexpr int CONV_ROWS = 32;           // ... and its output rows
constexpr int CONV_ROUND = 2 * MAX_RADIUS + 1;      // taps per staging round of the vertical pass

__global__ __launch_bounds__(256) void conv_rows_kernel(
    const float *__restrict__ in, int64_t in_row_pitch, int64_t in_pol_pitch,
    float *__restrict__ out, int64_t out_row_pitch, int64_t out_pol_pitch,
    int width, int height, const float *__restrict__ taps, int R)
{
    __shared__ float s_in[CONV_ROW + 2 * CONV_MAX_RADIUS];
    __shared__ float s_taps[2 * CONV_MAX_RADIUS + 1];
    const int tid = threadIdx.x, y = blockIdx.y, x0 = blockIdx.x * CONV_ROW;
    const float *row = in + blockIdx.z * in_pol_pitch + (int64_t) y * in_row_pitch;
    for (int i = tid; i < CONV_ROW + 2 * R; i += 256) {
        const int x = x0 - R + i;
        s_in[i] = x >= 0 && x < width ? row[x] : 0.0f;
    }
    for (int i = tid; i <= 2 * R; i += 256)
        s_taps[i] = taps[i];
    __syncthreads();
    const int x = x0 + tid;
    if (x >= width)
        return;
    const int lo = max(0, R - x), hi = min(2 * R, R + width - 1 - x);
    float acc = 0.0f;
    for (int i = lo; i <= hi; i++)
        acc = acc + s_taps[i] * s_in[tid + i];
    out[blockIdx.z * out_pol_pitch + (int64_t) y * out_row_pitch + x] = acc;
}

// The vertical pass walks the image in strips of 64 columns: a wave reads and writes 64 consecutive
// floats of a row, and the rows a workgroup needs are staged in LDS, CONV_ROUND taps' worth at a
// time (the sums stay in registers between the rounds, so the order of the additions is kept).
__global__ __launch_bounds__(256) void conv_columns_kernel(
    const float *__restrict__ in, int64_t in_row_pitch, int64_t in_pol_pitch,
    float *__restrict__ out, int64_t out_row_pitch, int64_t out_pol_pitch,
    int width, int height, const float *__restrict__ taps, int R)
{
    __shared__ float s_in[(CONV_ROWS + CONV_ROUND - 1) * CONV_STRIP];     // 40 KiB
    __shared__ float s_taps[2 * CONV_MAX_RADIUS + 1];
    const int tid = threadIdx.x, lane = tid & 63, sub = tid >> 6;
    const int x = blockIdx.x * CONV_STRIP + lane, y0 = blockIdx.y * CONV_ROWS;
    const float *plane = in + blockIdx.z * in_pol_pitch;
    for (int i = tid; i <= 2 * R; i += 256)
        s_taps[i] = taps[i];
    float acc[CONV_ROWS / 4];
#pragma unroll
    for (int m = 0; m < CONV_ROWS / 4; m++)
        acc[m] = 0.0f;
    for (int c0 = 0; c0 <= 2 * R; c0 += CONV_ROUND) {
        const int nt = min(CONV_ROUND, 2 * R + 1 - c0);
        __syncthreads();                // (the taps; the reads of the round before)
        for (int r = sub; r < CONV_ROWS + nt - 1; r += 4) {
            const int y = y0 - R + c0 + r;
            s_in[r * CONV_STRIP + lane] =
                x < width && y >= 0 && y < height ? plane[(int64_t) y * in_row_pitch + x] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < CONV_ROWS / 4; m++) {
            const int r = sub + 4 * m, y = y0 + r;
            const int lo = max(c0, R - y), hi = min(c0 + nt - 1, R + height - 1 - y);
            if (y < height)
                for (int i = lo; i <= hi; i++)
                    acc[m] = acc[m] + s_taps[i] * s_in[(r + i - c0) * CONV_STRIP + lane];
        }
    }
    if (x >= width)
        return;
#pragma unroll
    for (int m = 0; m < CONV_ROWS / 4; m++) {
        const int y = y0 + sub + 4 * m;
        if (y < height)
            out[blockIdx.z * out_pol_pitch + (int64_t) y * out_row_pitch + x] = acc[m];
    }
}

int convolve(const float *in, int64_t in_row_pitch, int64_t in_pol_pitch,
             float *out, int64_t out_row_pitch, int64_t out_pol_pitch,
             float *tmp, int64_t tmp_row_pitch, int64_t tmp_pol_pitch,
             int width, int height, int P, const float *taps, int R, hipStream_t s)
{
    conv_rows_kernel<<<dim3(kimg_divup(width, CONV_ROW), height, P), 256, 0, s>>>(
        in, in_row_pitch, in_pol_pitch, tmp, tmp_row_pitch, tmp_pol_pitch, width, height, taps, R);
    conv_columns_kernel<<<dim3(kimg_divup(width, CONV_STRIP), kimg_divup(height, CONV_ROWS), P), 256, 0, s>>>(
        tmp, tmp_row_pitch, tmp_pol_pitch, out, out_row_pitch, out_pol_pitch, width, height, taps, R);
    return kimg_launch_status();
}

// ---- set-up -----------------------------------------------------------------------------------
// n[k] = value of the convolved PSF at the centre of polarization 0, inv[k] = 1.0f / n[k]
__global__ void norm_kernel(const float *__restrict__ centre, float *__restrict__ coef, int k)
{
    const float n = *centre;
    coef[k] = n;
    coef[8 + k] = 1.0f / n;
}

// out[p][y][x] = in[p][y0 + y][x0 + x] * *factor (a rounded multiply), w x h pixels of P planes
__global__ __launch_bounds__(256) void crop_scale_kernel(
    const float *__restrict__ in, int64_t in_row_pitch, int64_t in_pol_pitch, int x0, int y0,
    float *__restrict__ out, int64_t out_row_pitch, int64_t out_pol_pitch, int w, int h,
    const float *__restrict__ factor)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h)
        return;
    const float f = *factor;
    out[blockIdx.z * out_pol_pitch + (int64_t) y * out_row_pitch + x] =
        in[blockIdx.z * in_pol_pitch + (int64_t) (y0 + y) * in_row_pitch + (x0 + x)] * f;
}

// ---- the minor cycle --------------------------------------------------------------------------
struct scales_state {
    int count;          // cycles completed
    int done;           // set once the loop has ended: every later launch of the call returns at once
    int limit;          // cycles this call may take
    float threshold;
    int active;         // the peak kernel of this cycle took a component: the update kernel runs
    int k;              // its scale
    int pos_y, pos_x;
    float a[4];         // loop_gain * residual of scale k at the peak, per polarization
};

// What a launch needs to know of the operator (a kernel argument, by value)
struct scales_desc {
    float *res[MAX_SCALES];             // residual of every scale; res[0] is the caller's dirty image
    int64_t res_row[MAX_SCALES], res_pol[MAX_SCALES];
    const float *cross;                 // cross patches: cross + cross_off[j * K + k] is X_jk
    int64_t cross_off[MAX_SCALES * MAX_SCALES];
    const float *taps;                  // taps of scale k at taps + k * TAPS_PITCH
    float *tile_max;                    // [K][tile_pitch]
    int32_t *tile_pos;                  // [K][tile_pitch][2]
    int64_t tile_pitch;
    int radius[MAX_SCALES];
    float bias[MAX_SCALES];
    int K, P, width, height, patch_w, patch_h, border, tiles_x, tiles_y;
    const uint8_t *mask;                // or null
    int64_t mask_row;
};

// The centred box of (patch + 2 R) pixels of an axis of n pixels, clipped to it: [lo, hi)
__host__ __device__ inline void crop_range(int n, int patch, int R, int &lo, int &hi)
{
    const int size = patch + 2 * R, start = n / 2 - size / 2;
    lo = start > 0 ? start : 0;
    hi = start + size < n ? start + size : n;
}

// Record of tile (tx, ty) of scale k from the four pixels (value, candidate) each of the 256
// threads holds: thread t has the pixels 4 t .. 4 t + 3 of the tile in row-major order.
__device__ inline void write_tile(const scales_desc &d, int k, int tx, int ty, const float v[4],
                                  const bool candidate[4], key_t *s_keys)
{
    const int tid = threadIdx.x;
    key_t key = 0;                      // only values above 0 count
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const float m = fabsf(v[e]);
        if (candidate[e] && m > 0.0f)
            key = key_max(key, make_key(m, 4 * tid + e));
    }
    key = block_max_key(key, s_keys);
    if (tid == 0) {
        const int64_t t = k * d.tile_pitch + (int64_t) ty * d.tiles_x + tx;
        store_tile_record(key, tx * TILE + d.border, ty * TILE + d.border, d.tile_max, d.tile_pos, t);
    }
}

__device__ inline bool is_candidate(const scales_desc &d, int x, int y)
{
    return x >= d.border && x < d.width - d.border && y >= d.border && y < d.height - d.border
           && (!d.mask || d.mask[(int64_t) y * d.mask_row + x]);
}

// Every tile of every scale: grid (tiles_x, tiles_y, K)
__global__ __launch_bounds__(256) void scales_tiles_kernel(scales_desc d)
{
    __shared__ key_t s_keys[4];
    const int k = blockIdx.z, tid = threadIdx.x;
    const int y = blockIdx.y * TILE + d.border + (tid >> 3);
    const int x4 = blockIdx.x * TILE + d.border + (tid & 7) * 4;
    float v[4];
    bool candidate[4];
    for (int e = 0; e < 4; e++) {
        candidate[e] = is_candidate(d, x4 + e, y);
        v[e] = candidate[e] ? d.res[k][(int64_t) y * d.res_row[k] + x4 + e] : 0.0f;
    }
    write_tile(d, k, blockIdx.x, blockIdx.y, v, candidate, s_keys);
}

__global__ void scales_init_kernel(scales_state *state, int limit, float threshold)
{
    state->count = 0;
    state->done = 0;
    state->limit = limit;
    state->threshold = threshold;
    state->active = 0;
}

// One workgroup: the peak of every scale from its tile records, the choice of the scale, the
// stopping rule, the component and its log entry.
__global__ __launch_bounds__(1024) void scales_peak_kernel(scales_desc d, scales_state *state,
                                                           float loop_gain, float *__restrict__ log)
{
    __shared__ key_t s_keys[MAX_SCALES][16];
    const int tid = threadIdx.x;
    if (state->done) {
        return;                 // (active is 0 since the cycle that set done)
    }
    const int num_tiles = d.tiles_x * d.tiles_y;
    for (int k = 0; k < d.K; k++) {
        key_t best = 0;
        for (int t = tid; t < num_tiles; t += 1024)
            best = key_max(best, make_key(d.tile_max[k * d.tile_pitch + t], t));
        best = wave_max_key(best);
        if ((tid & 63) == 0)
            s_keys[k][tid >> 6] = best;
    }
    __syncthreads();
    if (tid != 0)
        return;
    state->active = 0;
    if (state->count >= state->limit) {
        state->done = 1;
        return;
    }
    int ks = -1, ts = 0;
    float peak = 0.0f, biased = 0.0f;
    for (int k = 0; k < d.K; k++) {
        key_t best = 0;
        for (int w = 0; w < 16; w++)
            best = s_keys[k][w] > best ? s_keys[k][w] : best;
        const float v = __uint_as_float((unsigned) (best >> 32));
        const float b = d.bias[k] * v;
        if (ks < 0 || b > biased) {         // ties go to the smallest scale
            ks = k;
            ts = ~(int) (unsigned) best;
            peak = v;
            biased = b;
        }
    }
    if (peak < state->threshold || (d.mask && peak == 0.0f)) {
        state->done = 1;
        return;
    }
    const int64_t t = ks * d.tile_pitch + ts;
    const int y = d.tile_pos[2 * t], x = d.tile_pos[2 * t + 1];
    const int count = state->count;
    float *entry = log + (int64_t) count * (4 + d.P);
    for (int p = 0; p < d.P; p++) {
        const float a = loop_gain * d.res[ks][p * d.res_pol[ks] + (int64_t) y * d.res_row[ks] + x];
        state->a[p] = a;
        entry[4 + p] = a;
    }
    entry[0] = __int_as_float(ks);
    entry[1] = __int_as_float(y);
    entry[2] = __int_as_float(x);
    entry[3] = peak;
    state->k = ks;
    state->pos_y = y;
    state->pos_x = x;
    state->count = count + 1;
    state->active = 1;
}

// Steps 5 to 7 of a cycle in one launch.  blockIdx.z = j * P + p.  For j < K: workgroup
// (blockIdx.x, blockIdx.y) owns one 32 x 32 block of the tile lattice among those the box of scale
// j can touch; it subtracts a[p] * X_j,k* from the pixels of its block that lie in the box and,
// for polarization 0 of a block that is a tile, writes the tile's new record from the values it
// holds.  For j == K: the model, in 32 x 32 blocks of the component's (2 R + 1)^2 box.  Every
// pixel has one owner: no atomics.
__global__ __launch_bounds__(256) void scales_update_kernel(scales_desc d, const scales_state *state,
                                                            float *__restrict__ model)
{
    __shared__ key_t s_keys[4];
    if (!state->active)
        return;
    const int tid = threadIdx.x;
    const int j = blockIdx.z / d.P, p = blockIdx.z % d.P;
    const int ks = state->k, py = state->pos_y, px = state->pos_x;
    const float a = state->a[p];
    const int row = tid >> 3, col = (tid & 7) * 4;
    if (j == d.K) {
        const int R = d.radius[ks], n = 2 * R + 1;
        const float *taps = d.taps + ks * TAPS_PITCH;
        const int dy = blockIdx.y * TILE + row;
        const int y = py - R + dy;
        if (dy >= n || y < 0 || y >= d.height)
            return;
        for (int e = 0; e < 4; e++) {
            const int dx = blockIdx.x * TILE + col + e, x = px - R + dx;
            if (dx < n && x >= 0 && x < d.width) {
                const float w = taps[dy] * taps[dx];
                float *m = model + p * d.res_pol[0] + (int64_t) y * d.res_row[0] + x;
                *m = *m + a * w;
            }
        }
        return;
    }
    const int R = d.radius[j] + d.radius[ks];
    const int bw = d.patch_w + 2 * R, bh = d.patch_h + 2 * R;
    const int bx0 = px - bw / 2, by0 = py - bh / 2;
    // the lattice block: floor((b0 - border) / 32) + blockIdx
    const int fx = bx0 - d.border, fy = by0 - d.border;
    const int lx = (fx >= 0 ? fx / TILE : -((-fx + TILE - 1) / TILE)) + (int) blockIdx.x;
    const int ly = (fy >= 0 ? fy / TILE : -((-fy + TILE - 1) / TILE)) + (int) blockIdx.y;
    const int X0 = d.border + lx * TILE, Y0 = d.border + ly * TILE;
    if (X0 >= bx0 + bw || Y0 >= by0 + bh || X0 + TILE <= 0 || Y0 + TILE <= 0
        || X0 >= d.width || Y0 >= d.height)
        return;
    int cx0, cx1, cy0, cy1;             // the part of the convolved PSF that X holds
    crop_range(d.width, d.patch_w, R, cx0, cx1);
    crop_range(d.height, d.patch_h, R, cy0, cy1);
    const int cw = cx1 - cx0, ch = cy1 - cy0;
    const float *X = d.cross + d.cross_off[j * d.K + ks] + (int64_t) p * cw * ch;
    float *plane = d.res[j] + p * d.res_pol[j];
    const int y = Y0 + row, x4 = X0 + col;
    const bool row_ok = y >= 0 && y < d.height;
    float *ptr = plane + (int64_t) y * d.res_row[j] + x4;
    const bool vec = row_ok && x4 >= 0 && x4 + 3 < d.width
                     && (reinterpret_cast<uintptr_t>(ptr) & 15) == 0;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    bool changed[4] = {false, false, false, false};
    if (vec) {
        const float4 q = *reinterpret_cast<const float4 *>(ptr);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else if (row_ok) {
        for (int e = 0; e < 4; e++)
            if (x4 + e >= 0 && x4 + e < d.width)
                v[e] = ptr[e];
    }
    const int qy = d.height / 2 + (y - py);
    if (row_ok && y >= by0 && y < by0 + bh && qy >= cy0 && qy < cy1) {
        for (int e = 0; e < 4; e++) {
            const int x = x4 + e, qx = d.width / 2 + (x - px);
            if (x >= 0 && x < d.width && x >= bx0 && x < bx0 + bw && qx >= cx0 && qx < cx1) {
                v[e] = v[e] - a * X[(int64_t) (qy - cy0) * cw + (qx - cx0)];
                changed[e] = true;
            }
        }
    }
    if (vec) {
        if (changed[0] || changed[1] || changed[2] || changed[3])
            *reinterpret_cast<float4 *>(ptr) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int e = 0; e < 4; e++)
            if (changed[e])
                ptr[e] = v[e];
    }
    if (p != 0 || lx < 0 || lx >= d.tiles_x || ly < 0 || ly >= d.tiles_y)
        return;
    bool candidate[4];
    for (int e = 0; e < 4; e++)
        candidate[e] = is_candidate(d, x4 + e, y);
    write_tile(d, j, lx, ly, v, candidate, s_keys);
}

// ---- the workspace ----------------------------------------------------------------------------
// Sections in units of floats, each a multiple of 64 (256 bytes); see include/kimg.h.
struct layout_t {
    int64_t state, coef, taps, cross_taps, tile_max, tile_pos, res[MAX_SCALES],
            cross[MAX_SCALES * MAX_SCALES], tmp1, tmp2, total;
    int64_t tile_pitch;
    int tiles_x, tiles_y;
};

int64_t round64(int64_t n) { return (n + 63) / 64 * 64; }

bool make_layout(int width, int height, int P, int patch_w, int patch_h, int border, int K,
                 const int *radii, layout_t &l)
{
    if (width < 1 || height < 1 || P < 1 || P > 4 || patch_w < 1 || patch_h < 1
        || patch_w > width || patch_h > height || border < 0
        || 2 * border >= width || 2 * border >= height || K < 1 || !radii)
        return false;
    l.tiles_x = kimg_divup(width - 2 * border, TILE);
    l.tiles_y = kimg_divup(height - 2 * border, TILE);
    l.tile_pitch = round64((int64_t) l.tiles_x * l.tiles_y);
    const int64_t image = round64((int64_t) P * height * width);
    int64_t at = 0;
    l.state = at; at += 64;
    l.coef = at; at += 64;
    l.taps = at; at += MAX_SCALES * TAPS_PITCH;
    l.cross_taps = at; at += round64(MAX_PAIRS * CROSS_PITCH);
    l.tile_max = at; at += K * l.tile_pitch;
    l.tile_pos = at; at += 2 * K * l.tile_pitch;
    l.res[0] = -1;
    for (int k = 1; k < K; k++) {
        l.res[k] = at;
        at += image;
    }
    for (int j = 0; j < K; j++)
        for (int k = 0; k < K; k++) {
            int x0, x1, y0, y1;
            crop_range(width, patch_w, radii[j] + radii[k], x0, x1);
            crop_range(height, patch_h, radii[j] + radii[k], y0, y1);
            l.cross[j * K + k] = at;
            at += round64((int64_t) P * (y1 - y0) * (x1 - x0));
        }
    l.tmp1 = at; at += image;
    l.tmp2 = at; at += image;
    l.total = at;
    return true;
}

// KIMG_EUNSUPPORTED for what the operator refuses, KIMG_EINVAL for nonsense
int check_scales(int K, const int *radii)
{
    KIMG_CHECK_ARG(K >= 1 && radii);
    if (K > MAX_SCALES)
        return KIMG_EUNSUPPORTED;
    for (int k = 0; k < K; k++) {
        KIMG_CHECK_ARG(radii[k] >= 0);
        if (radii[k] > MAX_RADIUS)
            return KIMG_EUNSUPPORTED;
    }
    KIMG_CHECK_ARG(radii[0] == 0);
    return 0;
}

void fill_desc(scales_desc &d, const layout_t &l, float *ws, float *dirty, int64_t row_pitch,
               int64_t pol_pitch, int width, int height, int P, int patch_w, int patch_h,
               int border, int K, const int *radii, const float *biases, const uint8_t *mask,
               int64_t mask_row_pitch)
{
    memset(&d, 0, sizeof(d));
    for (int k = 0; k < K; k++) {
        d.res[k] = k == 0 ? dirty : ws + l.res[k];
        d.res_row[k] = k == 0 ? row_pitch : width;
        d.res_pol[k] = k == 0 ? pol_pitch : (int64_t) height * width;
        d.radius[k] = radii[k];
        d.bias[k] = biases ? biases[k] : 1.0f;
    }
    d.cross = ws;
    for (int i = 0; i < K * K; i++)
        d.cross_off[i] = l.cross[i];
    d.taps = ws + l.taps;
    d.tile_max = ws + l.tile_max;
    d.tile_pos = reinterpret_cast<int32_t *>(ws + l.tile_pos);
    d.tile_pitch = l.tile_pitch;
    d.K = K; d.P = P; d.width = width; d.height = height;
    d.patch_w = patch_w; d.patch_h = patch_h; d.border = border;
    d.tiles_x = l.tiles_x; d.tiles_y = l.tiles_y;
    d.mask = mask;
    d.mask_row = mask_row_pitch;
}

}  // namespace

extern "C" int kimg_image_convolve_separable(
    const float *in, int64_t in_row_pitch, int64_t in_pol_pitch,
    float *out, int64_t out_row_pitch, int64_t out_pol_pitch,
    float *tmp, int64_t tmp_row_pitch, int64_t tmp_pol_pitch,
    int width, int height, int num_polarizations, const float *taps, int radius, void *stream)
{
    KIMG_CHECK_ARG(in && out && tmp && taps && width >= 1 && height >= 1);
    KIMG_CHECK_ARG(num_polarizations >= 1 && num_polarizations <= 4 && radius >= 0);
    KIMG_CHECK_ARG(in_row_pitch >= width && out_row_pitch >= width && tmp_row_pitch >= width);
    KIMG_CHECK_ARG(tmp != in && tmp != out);
    if (radius > MAX_RADIUS)
        return KIMG_EUNSUPPORTED;
    return convolve(in, in_row_pitch, in_pol_pitch, out, out_row_pitch, out_pol_pitch,
                    tmp, tmp_row_pitch, tmp_pol_pitch, width, height, num_polarizations, taps,
                    radius, (hipStream_t) stream);
}

extern "C" size_t kimg_clean_scales_workspace_bytes(int width, int height, int num_polarizations,
                                                    int patch_width, int patch_height, int border,
                                                    int num_scales, const int *radii)
{
    layout_t l;
    if (check_scales(num_scales, radii) != 0
        || !make_layout(width, height, num_polarizations, patch_width, patch_height, border,
                        num_scales, radii, l))
        return 0;
    return (size_t) l.total * sizeof(float);
}

extern "C" int kimg_clean_scales_setup(
    float *dirty, int64_t row_pitch, int64_t pol_pitch,
    const float *psf, int64_t psf_row_pitch, int64_t psf_pol_pitch,
    int width, int height, int num_polarizations, int patch_width, int patch_height, int border,
    int num_scales, const int *radii, const float *taps_host, const float *cross_taps_host,
    int what, const uint8_t *mask, int64_t mask_row_pitch,
    void *workspace, size_t workspace_bytes, void *stream)
{
    const int K = num_scales, P = num_polarizations;
    if (int rc = check_scales(K, radii))
        return rc;
    KIMG_CHECK_ARG(dirty && psf && taps_host && cross_taps_host && workspace);
    KIMG_CHECK_ARG(row_pitch >= width && psf_row_pitch >= width);
    KIMG_CHECK_ARG(!mask || mask_row_pitch >= width);
    KIMG_CHECK_ARG(what >= 1 && what <= 3);
    KIMG_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0);
    layout_t l;
    KIMG_CHECK_ARG(make_layout(width, height, P, patch_width, patch_height, border, K, radii, l));
    if (workspace_bytes < (size_t) l.total * sizeof(float))
        return KIMG_EWORKSPACE;
    hipStream_t s = (hipStream_t) stream;
    float *ws = static_cast<float *>(workspace);
    const int64_t plane = (int64_t) height * width;
    float *tmp1 = ws + l.tmp1, *tmp2 = ws + l.tmp2, *coef = ws + l.coef;
    if (what & KIMG_CLEAN_SCALES_PSF) {
        // the centre of the PSF must be exactly 1: the residual of scale 0 is the dirty image itself
        float centre = 0.0f;
        KIMG_HIP(hipMemcpyAsync(&centre, psf + (int64_t) (height / 2) * psf_row_pitch + width / 2,
                                sizeof(float), hipMemcpyDeviceToHost, s));
        KIMG_HIP(hipStreamSynchronize(s));
        KIMG_CHECK_ARG(centre == 1.0f);
        KIMG_HIP(hipMemcpyAsync(ws + l.taps, taps_host, (size_t) K * TAPS_PITCH * sizeof(float),
                                hipMemcpyHostToDevice, s));
        KIMG_HIP(hipMemcpyAsync(ws + l.cross_taps, cross_taps_host,
                                (size_t) K * (K + 1) / 2 * CROSS_PITCH * sizeof(float),
                                hipMemcpyHostToDevice, s));
        // the diagonal first: it makes the factors the other patches need
        for (int pass = 0; pass < 2; pass++) {
            int pair = 0;
            for (int j = 0; j < K; j++)
                for (int k = j; k < K; k++, pair++) {
                    if ((j == k) != (pass == 0))
                        continue;
                    const int R = radii[j] + radii[k];
                    if (int rc = convolve(psf, psf_row_pitch, psf_pol_pitch, tmp2, width, plane,
                                          tmp1, width, plane, width, height, P,
                                          ws + l.cross_taps + pair * CROSS_PITCH, R, s))
                        return rc;
                    if (j == k)
                        norm_kernel<<<1, 1, 0, s>>>(tmp2 + (int64_t) (height / 2) * width + width / 2,
                                                    coef, k);
                    int x0, x1, y0, y1;
                    crop_range(width, patch_width, R, x0, x1);
                    crop_range(height, patch_height, R, y0, y1);
                    const int cw = x1 - x0, ch = y1 - y0;
                    const dim3 grid(kimg_divup(cw, 64), kimg_divup(ch, 4), P);
                    crop_scale_kernel<<<grid, 256, 0, s>>>(
                        tmp2, width, plane, x0, y0, ws + l.cross[j * K + k], cw, (int64_t) cw * ch,
                        cw, ch, coef + 8 + j);
                    if (j != k)
                        crop_scale_kernel<<<grid, 256, 0, s>>>(
                            tmp2, width, plane, x0, y0, ws + l.cross[k * K + j], cw,
                            (int64_t) cw * ch, cw, ch, coef + 8 + k);
                }
        }
    }
    if (what & KIMG_CLEAN_SCALES_RESIDUALS) {
        for (int k = 1; k < K; k++) {
            if (int rc = convolve(dirty, row_pitch, pol_pitch, tmp2, width, plane, tmp1, width,
                                  plane, width, height, P, ws + l.taps + k * TAPS_PITCH, radii[k], s))
                return rc;
            crop_scale_kernel<<<dim3(kimg_divup(width, 64), kimg_divup(height, 4), P), 256, 0, s>>>(
                tmp2, width, plane, 0, 0, ws + l.res[k], width, plane, width, height, coef + 8 + k);
        }
        scales_desc d;
        fill_desc(d, l, ws, dirty, row_pitch, pol_pitch, width, height, P, patch_width,
                  patch_height, border, K, radii, nullptr, mask, mask_row_pitch);
        scales_tiles_kernel<<<dim3(l.tiles_x, l.tiles_y, K), 256, 0, s>>>(d);
    }
    return kimg_launch_status();
}

extern "C" int kimg_clean_scales_cycles(
    float *dirty, float *model, int64_t row_pitch, int64_t pol_pitch,
    int width, int height, int num_polarizations, int patch_width, int patch_height, int border,
    int mode, float loop_gain, float threshold, int num_scales, const int *radii,
    const float *biases, int max_cycles, const uint8_t *mask, int64_t mask_row_pitch,
    void *workspace, size_t workspace_bytes, float *log, int *cycles_done, void *stream)
{
    const int K = num_scales, P = num_polarizations;
    if (int rc = check_scales(K, radii))
        return rc;
    KIMG_CHECK_ARG(mode == KIMG_CLEAN_I || mode == KIMG_CLEAN_SUMSQ);
    if (mode != KIMG_CLEAN_I)
        return KIMG_EUNSUPPORTED;
    KIMG_CHECK_ARG(dirty && model && biases && workspace && log && cycles_done && max_cycles >= 0);
    KIMG_CHECK_ARG(row_pitch >= width);
    KIMG_CHECK_ARG(!mask || mask_row_pitch >= width);
    KIMG_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0);
    layout_t l;
    KIMG_CHECK_ARG(make_layout(width, height, P, patch_width, patch_height, border, K, radii, l));
    if (workspace_bytes < (size_t) l.total * sizeof(float))
        return KIMG_EWORKSPACE;
    hipStream_t s = (hipStream_t) stream;
    float *ws = static_cast<float *>(workspace);
    scales_state *state = reinterpret_cast<scales_state *>(ws + l.state);
    scales_desc d;
    fill_desc(d, l, ws, dirty, row_pitch, pol_pitch, width, height, P, patch_width, patch_height,
              border, K, radii, biases, mask, mask_row_pitch);
    int radius_max = 0;
    for (int k = 0; k < K; k++)
        radius_max = radii[k] > radius_max ? radii[k] : radius_max;
    // lattice blocks the largest box can touch (a box of n pixels meets at most n / 32 + 2)
    const dim3 grid((patch_width + 4 * radius_max) / TILE + 2, (patch_height + 4 * radius_max) / TILE + 2,
                    (K + 1) * P);
    *cycles_done = 0;
    scales_init_kernel<<<1, 1, 0, s>>>(state, max_cycles, threshold);
    int head[2] = {0, 0};
    for (int enqueued = 0; enqueued < max_cycles && !head[1];) {
        const int n = max_cycles - enqueued < CHUNK ? max_cycles - enqueued : CHUNK;
        for (int i = 0; i < n; i++) {
            scales_peak_kernel<<<1, 1024, 0, s>>>(d, state, loop_gain, log);
            scales_update_kernel<<<grid, 256, 0, s>>>(d, state, model);
        }
        enqueued += n;
        if (int rc = kimg_launch_status())
            return rc;
        // the one look at the device per chunk
        KIMG_HIP(hipMemcpyAsync(head, state, sizeof(head), hipMemcpyDeviceToHost, s));
        KIMG_HIP(hipStreamSynchronize(s));
    }
    *cycles_done = head[0];
    return kimg_launch_status();
}

KIMG_PRELOAD_THIS_UNIT(conv_rows_kernel)
