// CLEAN auto-masks (include/kimg.h, "CLEAN auto-masks"): a clean mask built on the device from the
// residual.  kimg_mask_threshold marks the pixels whose CLEAN metric stands above a threshold,
// kimg_mask_dilate grows such a seed mask by a Euclidean disk and combines it with other masks in
// the same pass.  Masks are uint8 [height][width], nonzero = allowed; every byte written here is 0
// or 1, and bytes of the row padding are never written.
#include "kimg_common.h"

namespace {

// ---- threshold ------------------------------------------------------------------------------------
constexpr int MT_THREADS = 256;

// The CLEAN metric (clean_metric<MODE> of clean.hip): |pol 0|, or the sum of squares in
// polarization order, every product and sum rounded on its own (-ffp-contract=off).
template <int MODE, int P>
__device__ inline float mask_metric(const float *__restrict__ pixel, int64_t pol_stride)
{
    if (MODE == KIMG_CLEAN_I)
        return fabsf(pixel[0]);
    float value = 0.0f;
    for (int p = 0; p < P; p++) {
        const float pix = pixel[p * pol_stride];
        value += pix * pix;
    }
    return value;
}

// One thread per group of four pixels of a row.  The groups of a row start where the row of the
// MASK is 4-byte aligned (shift = its address modulo 4), so that a whole group is one 32-bit store;
// the groups that hang over either end of the row are written byte by byte.  The image is read with
// 16-byte loads where the group's pixels are 16-byte aligned.
template <int MODE, int P>
__global__ __launch_bounds__(MT_THREADS)
void mask_threshold_kernel(const float *__restrict__ image, int64_t row_stride, int64_t pol_stride,
                           int width, int height, int border, float threshold,
                           uint8_t *__restrict__ mask, int64_t mask_row_stride, int groups_per_row)
{
    const int64_t i = (int64_t) blockIdx.x * MT_THREADS + threadIdx.x;
    if (i >= (int64_t) height * groups_per_row)
        return;
    const int y = (int) (i / groups_per_row);
    const int g = (int) (i % groups_per_row);
    uint8_t *mrow = mask + (int64_t) y * mask_row_stride;
    const int shift = (int) (reinterpret_cast<uintptr_t>(mrow) & 3);
    const int x0 = 4 * g - shift;
    if (x0 >= width || x0 + 4 <= 0)
        return;
    const bool row_inside = y >= border && y < height - border;
    const float *irow = image + (int64_t) y * row_stride;
    if (x0 >= 0 && x0 + 4 <= width) {
        uint32_t bytes = 0;
        if (row_inside && x0 + 4 > border && x0 < width - border) {
            float metric[4];
            const float *pixel = irow + x0;
            if ((reinterpret_cast<uintptr_t>(pixel) & 15) == 0 && (pol_stride & 3) == 0) {
                if (MODE == KIMG_CLEAN_I) {
                    const float4 v = *reinterpret_cast<const float4 *>(pixel);
                    metric[0] = fabsf(v.x);
                    metric[1] = fabsf(v.y);
                    metric[2] = fabsf(v.z);
                    metric[3] = fabsf(v.w);
                } else {
                    metric[0] = metric[1] = metric[2] = metric[3] = 0.0f;
                    for (int p = 0; p < P; p++) {
                        const float4 v = *reinterpret_cast<const float4 *>(pixel + p * pol_stride);
                        metric[0] += v.x * v.x;
                        metric[1] += v.y * v.y;
                        metric[2] += v.z * v.z;
                        metric[3] += v.w * v.w;
                    }
                }
            } else {
                for (int k = 0; k < 4; k++)
                    metric[k] = mask_metric<MODE, P>(pixel + k, pol_stride);
            }
            for (int k = 0; k < 4; k++) {
                const int x = x0 + k;
                if (x >= border && x < width - border && metric[k] > threshold)
                    bytes |= 1u << (8 * k);
            }
        }
        *reinterpret_cast<uint32_t *>(mrow + x0) = bytes;
    } else {
        for (int k = 0; k < 4; k++) {
            const int x = x0 + k;
            if (x < 0 || x >= width)
                continue;
            const bool inside = row_inside && x >= border && x < width - border;
            mrow[x] = inside && mask_metric<MODE, P>(irow + x, pol_stride) > threshold ? 1 : 0;
        }
    }
}

// ---- dilation -------------------------------------------------------------------------------------
// One workgroup owns a 64 x 64 tile of the output.
//   1. It stages the input bytes of the tile and of `radius` pixels around it in LDS (zeros outside
//      the plane), in aligned 32-bit words where the input allows.  A staged area without a set byte
//      skips steps 2 and 3 (sparse masks: most tiles).
//   2. One thread per staged row runs along the row once in each direction and leaves, for the
//      tile's 64 columns, the horizontal distance to the nearest set byte, capped at radius + 1.
//   3. A pixel is set where some |dy| <= radius has dist[y + dy][x] <= chord(dy), chord(dy) the
//      largest c with c^2 + dy^2 <= radius^2: exactly the disk, at 2 * radius + 1 looks per pixel.
//      A thread owns four columns (one 32-bit word of a dist row) of four rows that lie four rows
//      apart, reads every dist row it needs once, and compares the four bytes at once
//      ((0x80 + chord - dist) keeps bit 7 of a byte exactly where dist <= chord; no byte borrows,
//      for chord <= 64 and dist <= 65).
// LDS at radius 64: 192 rows x 196 bytes staged, 192 x 68 bytes of distances, 65 words of chords.
constexpr int MD_TILE = 64;
constexpr int MD_THREADS = 256;
constexpr int MD_DIST_STRIDE = MD_TILE + 4;     // bytes; 17 words: the rows' writers miss each other's banks

// Words per staged row: the tile, the radius on both sides and up to 3 bytes of alignment, rounded
// up to an odd number of words (one thread per row then reads conflict-free).
__host__ __device__ inline int md_stage_words(int radius)
{
    return ((MD_TILE + 2 * radius + 3 + 3) / 4) | 1;
}

__host__ __device__ inline size_t md_lds_bytes(int radius)
{
    const int rows = MD_TILE + 2 * radius;
    return (size_t) rows * md_stage_words(radius) * 4 + (size_t) rows * MD_DIST_STRIDE
           + (size_t) (radius + 1) * 4;
}

// 0 / 1 per byte: is the byte nonzero?
__device__ inline uint32_t nonzero_bytes(uint32_t w)
{
    return ((((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) >> 7) & 0x01010101u;
}

// Four bytes of row `row` from column x on, those outside [0, width) as 0; one 32-bit load where all
// four exist and are aligned.
__device__ inline uint32_t load_bytes4(const uint8_t *__restrict__ row, int x, int width)
{
    if (x >= 0 && x + 4 <= width && (reinterpret_cast<uintptr_t>(row + x) & 3) == 0)
        return *reinterpret_cast<const uint32_t *>(row + x);
    uint32_t w = 0;
    for (int k = 0; k < 4; k++)
        if (x + k >= 0 && x + k < width)
            w |= (uint32_t) row[x + k] << (8 * k);
    return w;
}

__global__ __launch_bounds__(MD_THREADS)
void mask_dilate_kernel(const uint8_t *__restrict__ in, int64_t in_row_stride,
                        uint8_t *out, int64_t out_row_stride, int width, int height, int radius,
                        const uint8_t *or_with, int64_t or_row_stride,
                        const uint8_t *__restrict__ and_with, int64_t and_row_stride,
                        uint32_t *__restrict__ count)
{
    extern __shared__ uint32_t md_lds[];
    __shared__ unsigned set_pixels;
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * MD_TILE, y0 = blockIdx.y * MD_TILE;
    const int rows = MD_TILE + 2 * radius;
    const int stage_words = md_stage_words(radius);
    uint32_t *stage = md_lds;                                           // [rows][stage_words]
    uint8_t *dist = reinterpret_cast<uint8_t *>(stage + rows * stage_words);   // [rows][MD_DIST_STRIDE]
    uint32_t *chord = reinterpret_cast<uint32_t *>(dist + rows * MD_DIST_STRIDE);   // [radius + 1]
    // staged column 0 is the plane's column gx0, at most 3 to the left of x0 - radius, where the
    // rows of `in` are 4-byte aligned (if its stride keeps them so)
    const int pad = (int) ((reinterpret_cast<uintptr_t>(in) + (uintptr_t) (int64_t) (x0 - radius)) & 3);
    const int gx0 = x0 - radius - pad;

    if (tid == 0)
        set_pixels = 0;
    if (tid <= radius) {
        // chord(dy): largest c with c^2 + dy^2 <= radius^2, as 0x80 + c in every byte
        const int left = radius * radius - tid * tid;
        int c = (int) sqrtf((float) left);
        while (c * c > left)
            c--;
        while ((c + 1) * (c + 1) <= left)
            c++;
        chord[tid] = 0x80808080u | (uint32_t) c * 0x01010101u;
    }
    uint32_t any = 0;
    for (int i = tid; i < rows * stage_words; i += MD_THREADS) {
        const int ry = i / stage_words, j = i - ry * stage_words;
        const int gy = y0 - radius + ry;
        uint32_t w = 0;
        if (gy >= 0 && gy < height)
            w = nonzero_bytes(load_bytes4(in + (int64_t) gy * in_row_stride, gx0 + 4 * j, width));
        stage[i] = w;
        any |= w;
    }
    const bool some = __syncthreads_or(any != 0);

    uint32_t acc[4] = {0, 0, 0, 0};
    const int lane = tid & 63, wave = tid >> 6;
    const int xg = lane & 15, sub = lane >> 4;
    if (some) {
        const int cap = radius + 1;
        if (tid < rows) {
            const uint32_t *srow = stage + tid * stage_words;
            uint8_t *drow = dist + tid * MD_DIST_STRIDE;
            const int first = radius + pad;         // staged column of the tile's column 0
            int d = cap;
            for (int w = 0; w < stage_words; w++) {
                const uint32_t word = srow[w];
                for (int k = 0; k < 4; k++) {
                    d = ((word >> (8 * k)) & 0xff) ? 0 : min(d + 1, cap);
                    const int x = 4 * w + k - first;
                    if (x >= 0 && x < MD_TILE)
                        drow[x] = (uint8_t) d;
                }
            }
            d = cap;
            for (int w = stage_words - 1; w >= 0; w--) {
                const uint32_t word = srow[w];
                for (int k = 3; k >= 0; k--) {
                    d = ((word >> (8 * k)) & 0xff) ? 0 : min(d + 1, cap);
                    const int x = 4 * w + k - first;
                    if (x >= 0 && x < MD_TILE && d < drow[x])
                        drow[x] = (uint8_t) d;
                }
            }
        }
        __syncthreads();
        // output rows wave * 16 + sub + 4 k (k = 0..3) of the tile; the dist row of output row y
        // and offset dy is staged row y + radius + dy
        const uint32_t *dist32 = reinterpret_cast<const uint32_t *>(dist);
        const int base = wave * 16 + sub;
        for (int j = 0; j <= 2 * radius + 12; j++) {
            const uint32_t word = dist32[(base + j) * (MD_DIST_STRIDE / 4) + xg];
            for (int k = 0; k < 4; k++) {
                const int dy = j - 4 * k - radius;
                if (dy >= -radius && dy <= radius)
                    acc[k] |= (chord[dy < 0 ? -dy : dy] - word) & 0x80808080u;
            }
        }
    }

    unsigned n = 0;
    const int gx = x0 + 4 * xg;
    for (int k = 0; k < 4; k++) {
        const int gy = y0 + wave * 16 + sub + 4 * k;
        uint32_t bytes = 0;
        const bool live = gy < height && gx < width;
        if (live) {
            bytes = acc[k] >> 7;
            if (or_with)
                bytes |= nonzero_bytes(load_bytes4(or_with + (int64_t) gy * or_row_stride, gx, width));
            if (and_with)
                bytes &= nonzero_bytes(load_bytes4(and_with + (int64_t) gy * and_row_stride, gx, width));
            uint8_t *orow = out + (int64_t) gy * out_row_stride;
            if (gx + 4 <= width && (reinterpret_cast<uintptr_t>(orow + gx) & 3) == 0) {
                *reinterpret_cast<uint32_t *>(orow + gx) = bytes;
            } else {
                for (int b = 0; b < 4; b++) {
                    if (gx + b < width)
                        orow[gx + b] = (uint8_t) ((bytes >> (8 * b)) & 1);
                    else
                        bytes &= ~(0xffu << (8 * b));
                }
            }
        }
        if (count)
            for (int b = 0; b < 4; b++)
                n += __popcll(__ballot((bytes >> (8 * b)) & 1));
    }
    if (count) {
        // n is the wave's: one LDS add per wave, one global atomic per workgroup
        if (lane == 0 && n)
            atomicAdd(&set_pixels, n);
        __syncthreads();
        if (tid == 0 && set_pixels)
            atomicAdd(count, set_pixels);
    }
}

}  // namespace

extern "C" int kimg_mask_threshold(const float *image, int64_t row_pitch, int64_t pol_pitch,
                                   int width, int height, int num_polarizations, int border,
                                   int mode, float threshold, uint8_t *mask,
                                   int64_t mask_row_pitch, void *stream)
{
    KIMG_CHECK_ARG(image && mask && width >= 1 && height >= 1 && border >= 0);
    KIMG_CHECK_ARG(num_polarizations >= 1 && num_polarizations <= 4);
    KIMG_CHECK_ARG(row_pitch >= width && mask_row_pitch >= width);
    KIMG_CHECK_ARG(mode == KIMG_CLEAN_I || mode == KIMG_CLEAN_SUMSQ);
    hipStream_t s = (hipStream_t) stream;
    const int groups_per_row = (width + 3) / 4 + 1;     // whatever the rows' alignment
    const unsigned blocks = (unsigned) kimg_divup((int64_t) height * groups_per_row, MT_THREADS);
    if (mode == KIMG_CLEAN_I) {
        mask_threshold_kernel<KIMG_CLEAN_I, 1><<<blocks, MT_THREADS, 0, s>>>(
            image, row_pitch, pol_pitch, width, height, border, threshold, mask, mask_row_pitch,
            groups_per_row);
    } else {
        kimg_for_pols(num_polarizations, [&](auto pols) {
            mask_threshold_kernel<KIMG_CLEAN_SUMSQ, decltype(pols)::value><<<blocks, MT_THREADS, 0, s>>>(
                image, row_pitch, pol_pitch, width, height, border, threshold, mask,
                mask_row_pitch, groups_per_row);
        });
    }
    return kimg_launch_status();
}

extern "C" int kimg_mask_dilate(const uint8_t *in, int64_t in_row_pitch, uint8_t *out,
                                int64_t out_row_pitch, int width, int height, int radius,
                                const uint8_t *or_with, int64_t or_row_pitch,
                                const uint8_t *and_with, int64_t and_row_pitch, uint32_t *count,
                                void *stream)
{
    KIMG_CHECK_ARG(in && out && width >= 1 && height >= 1);
    KIMG_CHECK_ARG(radius >= 0 && radius <= KIMG_MASK_MAX_RADIUS);
    KIMG_CHECK_ARG(in_row_pitch >= width && out_row_pitch >= width);
    KIMG_CHECK_ARG(!or_with || or_row_pitch >= width);
    KIMG_CHECK_ARG(!and_with || and_row_pitch >= width);
    // (or_with may be out: a thread reads its bytes before it writes them)
    KIMG_CHECK_ARG(in != out && and_with != out);
    hipStream_t s = (hipStream_t) stream;
    if (count)
        KIMG_HIP(hipMemsetAsync(count, 0, sizeof(uint32_t), s));
    const dim3 grid((unsigned) kimg_divup(width, MD_TILE), (unsigned) kimg_divup(height, MD_TILE));
    mask_dilate_kernel<<<grid, MD_THREADS, md_lds_bytes(radius), s>>>(
        in, in_row_pitch, out, out_row_pitch, width, height, radius, or_with, or_row_pitch,
        and_with, and_row_pitch, count);
    return kimg_launch_status();
}

KIMG_PRELOAD_THIS_UNIT(mask_dilate_kernel)
