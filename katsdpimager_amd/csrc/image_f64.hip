// Float64 image-plane kernels: the grid <-> layer quadrant copies, layer <-> image (fftshift +
// W-stack phase + n-term + taper), scale, add_image and apply_primary_beam on complex128 / float64
// arrays (the reference's --precision double).  Same operations, in the same order, as the float32
// kernels of image.hip; the phase comes from double sincospi after the same range reduction.
// Float64 always takes the plain route (copy, C2C transform, layer -> image): the library's own
// transforms and the w = 0 real route of image.hip are float32 only.
#include "kimg_common.h"

namespace {

__global__ __launch_bounds__(256) void grid_to_layer_f64_kernel(
    double2 *__restrict__ layer, int G, const double2 *__restrict__ grid, int64_t grid_row_stride,
    int Gg)
{
    const int lx = blockIdx.x * blockDim.x + threadIdx.x;
    const int ly = blockIdx.y;
    if (lx >= G)
        return;
    const int half = Gg / 2;
    const int cx = lx < G - half ? lx : lx - G;
    const int cy = ly < G - half ? ly : ly - G;
    double2 v = make_double2(0.0, 0.0);
    if (cx >= -half && cx < half && cy >= -half && cy < half)
        v = grid[(int64_t) (cy + half) * grid_row_stride + (cx + half)];
    layer[(int64_t) ly * G + lx] = v;
}

__global__ __launch_bounds__(256) void layer_to_grid_f64_kernel(
    double2 *__restrict__ grid, int64_t grid_row_stride, int Gg, const double2 *__restrict__ layer,
    int G)
{
    const int gx = blockIdx.x * blockDim.x + threadIdx.x;
    const int gy = blockIdx.y;
    if (gx >= Gg)
        return;
    const int half = Gg / 2;
    int lx = gx - half, ly = gy - half;
    if (lx < 0) lx += G;
    if (ly < 0) ly += G;
    grid[(int64_t) gy * grid_row_stride + gx] = layer[(int64_t) ly * G + lx];
}

// e^{2 pi i x}, reduced to |r| <= 1/2 turn first (fast_math.py:14-15)
__device__ inline void expj2pi_f64(double x, double &c, double &s)
{
    const double r = x - rint(x);
    sincospi(2.0 * r, &s, &c);
}

__device__ inline double n_term(int x, int y, double lm_scale, double lm_bias)
{
    const double l = (double) x * lm_scale + lm_bias;
    const double m = (double) y * lm_scale + lm_bias;
    return sqrt(1.0 - (m * m + l * l));
}

// image[y][x] += Re(layer[(y+G/2)%G][(x+G/2)%G] * e^{2 pi i w (n-1)}) * n / (k[y] k[x])
__global__ __launch_bounds__(256) void layer_to_image_f64_kernel(
    double *__restrict__ image, int64_t image_row_stride, const double2 *__restrict__ layer, int G,
    const double *__restrict__ kernel1d, double lm_scale, double lm_bias, double w)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= G)
        return;
    const int half = G / 2;
    const int sx = x < half ? x + half : x - half;
    const int sy = y < half ? y + half : y - half;
    const double2 v = layer[(int64_t) sy * G + sx];
    const double n = n_term(x, y, lm_scale, lm_bias);
    double c, s;
    expj2pi_f64(w * (n - 1.0), c, s);
    const double rotated = v.x * c - v.y * s;
    const double taper = kernel1d[y] * kernel1d[x];
    image[(int64_t) y * image_row_stride + x] += (rotated * n) / taper;
}

// layer[(y+G/2)%G][(x+G/2)%G] = image[y][x] / (k[y] k[x] n) * e^{-2 pi i w (n-1)}
__global__ __launch_bounds__(256) void image_to_layer_f64_kernel(
    double2 *__restrict__ layer, const double *__restrict__ image, int64_t image_row_stride, int G,
    const double *__restrict__ kernel1d, double lm_scale, double lm_bias, double w)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= G)
        return;
    const int half = G / 2;
    const int sx = x < half ? x + half : x - half;
    const int sy = y < half ? y + half : y - half;
    const double n = n_term(x, y, lm_scale, lm_bias);
    double c, s;
    expj2pi_f64(-w * (n - 1.0), c, s);
    const double taper = kernel1d[y] * kernel1d[x];
    const double v = image[(int64_t) y * image_row_stride + x] / (taper * n);
    layer[(int64_t) sy * G + sx] = make_double2(v * c, v * s);
}

struct scale_f64_t { double v[4]; };

__global__ __launch_bounds__(256) void scale_f64_kernel(
    double *__restrict__ image, int64_t row_stride, int64_t pol_stride, int width, int num_pols,
    scale_f64_t scale)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= width)
        return;
    int64_t addr = (int64_t) blockIdx.y * row_stride + x;
    for (int p = 0; p < num_pols; p++, addr += pol_stride)
        image[addr] *= scale.v[p];
}

__global__ __launch_bounds__(256) void add_image_f64_kernel(
    double *__restrict__ dest, int64_t dest_row_stride, int64_t dest_pol_stride,
    const double *__restrict__ src, int64_t src_row_stride, int64_t src_pol_stride,
    int width, int num_pols)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= width)
        return;
    int64_t d = (int64_t) blockIdx.y * dest_row_stride + x;
    int64_t s = (int64_t) blockIdx.y * src_row_stride + x;
    for (int p = 0; p < num_pols; p++, d += dest_pol_stride, s += src_pol_stride)
        dest[d] += src[s];
}

__global__ __launch_bounds__(256) void apply_primary_beam_f64_kernel(
    double *__restrict__ image, int64_t row_stride, int64_t pol_stride,
    const double *__restrict__ beam_power, int64_t beam_row_stride, int width, int num_pols,
    double threshold, double replacement)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= width)
        return;
    const double beam = beam_power[(int64_t) blockIdx.y * beam_row_stride + x];
    int64_t addr = (int64_t) blockIdx.y * row_stride + x;
    for (int p = 0; p < num_pols; p++, addr += pol_stride)
        image[addr] = beam < threshold ? replacement : image[addr] / beam;
}

} // namespace

extern "C" int kimg_grid_to_layer_f64(void *layer, int layer_size, const void *grid,
                                      int64_t grid_row_stride, int grid_size, void *stream)
{
    KIMG_CHECK_ARG(layer && grid && layer_size > 0 && grid_size > 0 && grid_size <= layer_size);
    KIMG_CHECK_ARG(layer_size % 2 == 0 && grid_size % 2 == 0 && grid_row_stride >= grid_size);
    const dim3 g(kimg_divup(layer_size, 256), layer_size);
    grid_to_layer_f64_kernel<<<g, 256, 0, (hipStream_t) stream>>>(
        (double2 *) layer, layer_size, (const double2 *) grid, grid_row_stride, grid_size);
    return kimg_launch_status();
}

extern "C" int kimg_layer_to_grid_f64(void *grid, int64_t grid_row_stride, int grid_size,
                                      const void *layer, int layer_size, void *stream)
{
    KIMG_CHECK_ARG(layer && grid && layer_size > 0 && grid_size > 0 && grid_size <= layer_size);
    KIMG_CHECK_ARG(layer_size % 2 == 0 && grid_size % 2 == 0 && grid_row_stride >= grid_size);
    const dim3 g(kimg_divup(grid_size, 256), grid_size);
    layer_to_grid_f64_kernel<<<g, 256, 0, (hipStream_t) stream>>>(
        (double2 *) grid, grid_row_stride, grid_size, (const double2 *) layer, layer_size);
    return kimg_launch_status();
}

extern "C" int kimg_layer_to_image_f64(double *image, int64_t image_row_stride, const void *layer,
                                       int size, const double *kernel1d, double lm_scale,
                                       double lm_bias, double w, void *stream)
{
    KIMG_CHECK_ARG(image && layer && kernel1d && size > 0 && size % 2 == 0
                   && image_row_stride >= size);
    const dim3 g(kimg_divup(size, 256), size);
    layer_to_image_f64_kernel<<<g, 256, 0, (hipStream_t) stream>>>(
        image, image_row_stride, (const double2 *) layer, size, kernel1d, lm_scale, lm_bias, w);
    return kimg_launch_status();
}

extern "C" int kimg_image_to_layer_f64(void *layer, const double *image, int64_t image_row_stride,
                                       int size, const double *kernel1d, double lm_scale,
                                       double lm_bias, double w, void *stream)
{
    KIMG_CHECK_ARG(image && layer && kernel1d && size > 0 && size % 2 == 0
                   && image_row_stride >= size);
    const dim3 g(kimg_divup(size, 256), size);
    image_to_layer_f64_kernel<<<g, 256, 0, (hipStream_t) stream>>>(
        (double2 *) layer, image, image_row_stride, size, kernel1d, lm_scale, lm_bias, w);
    return kimg_launch_status();
}

extern "C" int kimg_scale_f64(double *image, int64_t row_stride, int64_t pol_stride, int width,
                              int height, int num_polarizations, const double *scale_host,
                              void *stream)
{
    KIMG_CHECK_ARG(image && scale_host && width > 0 && height > 0);
    if (num_polarizations < 1 || num_polarizations > 4)
        return KIMG_EUNSUPPORTED;
    scale_f64_t sc = {};
    for (int p = 0; p < num_polarizations; p++)
        sc.v[p] = scale_host[p];
    const dim3 g(kimg_divup(width, 256), height);
    scale_f64_kernel<<<g, 256, 0, (hipStream_t) stream>>>(image, row_stride, pol_stride, width,
                                                          num_polarizations, sc);
    return kimg_launch_status();
}

extern "C" int kimg_add_image_f64(double *dest, int64_t dest_row_stride, int64_t dest_pol_stride,
                                  const double *src, int64_t src_row_stride,
                                  int64_t src_pol_stride, int width, int height,
                                  int num_polarizations, void *stream)
{
    KIMG_CHECK_ARG(dest && src && width > 0 && height > 0 && num_polarizations > 0);
    const dim3 g(kimg_divup(width, 256), height);
    add_image_f64_kernel<<<g, 256, 0, (hipStream_t) stream>>>(
        dest, dest_row_stride, dest_pol_stride, src, src_row_stride, src_pol_stride, width,
        num_polarizations);
    return kimg_launch_status();
}

extern "C" int kimg_apply_primary_beam_f64(double *image, int64_t row_stride, int64_t pol_stride,
                                           const double *beam_power, int64_t beam_row_stride,
                                           int width, int height, int num_polarizations,
                                           double threshold, double replacement, void *stream)
{
    KIMG_CHECK_ARG(image && beam_power && width > 0 && height > 0 && num_polarizations > 0);
    const dim3 g(kimg_divup(width, 256), height);
    apply_primary_beam_f64_kernel<<<g, 256, 0, (hipStream_t) stream>>>(
        image, row_stride, pol_stride, beam_power, beam_row_stride, width, num_polarizations,
        threshold, replacement);
    return kimg_launch_status();
}

// (kimg_preload, api.hip)
KIMG_PRELOAD_THIS_UNIT(grid_to_layer_f64_kernel)
