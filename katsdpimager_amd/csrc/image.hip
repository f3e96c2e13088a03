// Image-plane kernels: grid<->layer quadrant copies, layer<->image (fftshift + W-stack phase
// + n-term + taper), scale, add_image, apply_primary_beam.  All HBM-bound streams.
// Mirrors image.py:153-180, 351-367, 439-458, 539-558, 649-673, 716-740 of the reference.
// The arithmetic order follows the reference HOST classes (image.py:781-799, 836-848) so that
// float32 results agree to rounding; this file is built with -ffp-contract=off.
// (The library's own LDS transforms, and the entry points built on them, are in transform.hip.)
#include "kimg_common.h"
#include "kimg_layer_math.h"

namespace {

// The plain kernels below (grid <-> layer copies, layer <-> image, scale, add_image,
// apply_primary_beam) are templates on the real type T: float for the float32 entry points,
// double for the *_f64 ones.  cplx<T> is the complex cell that goes with it.
template <typename T> struct cplx_of;
template <> struct cplx_of<float> { using type = float2; };
template <> struct cplx_of<double> { using type = double2; };
template <typename T> using cplx = typename cplx_of<T>::type;

// layer[ly][lx] = grid cell with the same (centred) frequency, or 0 outside the grid.
// Fuses the reference's layer.zero() + 4 copy_region calls (image.py:660-671).
template <typename T>
__global__ __launch_bounds__(256) void grid_to_layer_kernel(
    cplx<T> *__restrict__ layer, int G, const cplx<T> *__restrict__ grid, int64_t grid_row_stride,
    int Gg)
{
    const int lx = blockIdx.x * blockDim.x + threadIdx.x;
    const int ly = blockIdx.y;
    if (lx >= G)
        return;
    const int half = Gg / 2;
    // centred coordinates of this layer pixel: 0..G/2-1 positive, G/2.. negative
    const int cx = lx < G - half ? lx : lx - G;
    const int cy = ly < G - half ? ly : ly - G;
    cplx<T> v(T(0), T(0));
    if (cx >= -half && cx < half && cy >= -half && cy < half)
        v = grid[(int64_t) (cy + half) * grid_row_stride + (cx + half)];
    layer[(int64_t) ly * G + lx] = v;
}

// The same for a transform that is only wanted for its REAL part: the Hermitian half of the layer
// (half_layer_value, kimg_layer_math.h), half[ly][lx], row length G/2 + 1.
__global__ __launch_bounds__(256) void grid_to_half_layer_kernel(
    float2 *__restrict__ half_layer, int G, const float2 *__restrict__ grid,
    int64_t grid_row_stride, int Gg)
{
    const int lx = blockIdx.x * blockDim.x + threadIdx.x;
    const int ly = blockIdx.y;
    const int W = G / 2 + 1;
    if (lx >= W)
        return;
    half_layer[(int64_t) ly * W + lx] = half_layer_value(grid, grid_row_stride, Gg, G, lx, ly);
}

template <typename T>
__global__ __launch_bounds__(256) void layer_to_grid_kernel(
    cplx<T> *__restrict__ grid, int64_t grid_row_stride, int Gg, const cplx<T> *__restrict__ layer,
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

// One thread: one image pixel pair... kept simple: one pixel per thread, x fastest.
// image[y][x] += Re(layer[(y+G/2)%G][(x+G/2)%G] * e^{2 pi i w (n-1)}) * n / (k[y] k[x])
template <typename T>
__global__ __launch_bounds__(256) void layer_to_image_kernel(
    T *__restrict__ image, int64_t image_row_stride, const cplx<T> *__restrict__ layer, int G,
    const T *__restrict__ kernel1d, T lm_scale, T lm_bias, T w)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= G)
        return;
    const int half = G / 2;
    const int sx = x < half ? x + half : x - half;
    const int sy = y < half ? y + half : y - half;
    const cplx<T> v = layer[(int64_t) sy * G + sx];
    const T l = lm_coord(x, lm_scale, lm_bias);
    const T m = lm_coord(y, lm_scale, lm_bias);
    const T n = real_sqrt(T(1) - (m * m + l * l));
    T c, s;
    expj2pi(w * (n - T(1)), c, s);
    const T rotated = v.x * c - v.y * s;
    const T taper = kernel1d[y] * kernel1d[x];
    image[(int64_t) y * image_row_stride + x] += (rotated * n) / taper;
}

// layer_to_image for w = 0 from the real output of the complex-to-real transform (rows of
// `layer_row_stride` floats): the phase factor is exactly (1, 0), so "rotated" is the real part.
__global__ __launch_bounds__(256) void real_layer_to_image_kernel(
    float *__restrict__ image, int64_t image_row_stride, const float *__restrict__ layer,
    int64_t layer_row_stride, int G, const float *__restrict__ kernel1d, float lm_scale, float lm_bias)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= G)
        return;
    const int half = G / 2;
    const int sx = x < half ? x + half : x - half;
    const int sy = y < half ? y + half : y - half;
    const float rotated = layer[(int64_t) sy * layer_row_stride + sx];
    const float l = lm_coord(x, lm_scale, lm_bias);
    const float m = lm_coord(y, lm_scale, lm_bias);
    const float l2 = l * l, m2 = m * m;
    const float n = sqrtf(1.0f - (m2 + l2));
    const float taper = kernel1d[y] * kernel1d[x];
    image[(int64_t) y * image_row_stride + x] += (rotated * n) / taper;
}

// layer[(y+G/2)%G][(x+G/2)%G] = image[y][x] / (k[y] k[x] n) * e^{-2 pi i w (n-1)}
template <typename T>
__global__ __launch_bounds__(256) void image_to_layer_kernel(
    cplx<T> *__restrict__ layer, const T *__restrict__ image, int64_t image_row_stride, int G,
    const T *__restrict__ kernel1d, T lm_scale, T lm_bias, T w)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= G)
        return;
    const int half = G / 2;
    const int sx = x < half ? x + half : x - half;
    const int sy = y < half ? y + half : y - half;
    const T l = lm_coord(x, lm_scale, lm_bias);
    const T m = lm_coord(y, lm_scale, lm_bias);
    const T n = real_sqrt(T(1) - (m * m + l * l));
    T c, s;
    expj2pi(-w * (n - T(1)), c, s);
    const T taper = kernel1d[y] * kernel1d[x];
    const T v = image[(int64_t) y * image_row_stride + x] / (taper * n);
    layer[(int64_t) sy * G + sx] = cplx<T>(v * c, v * s);
}

// image_to_layer for w = 0: the layer is real (phase factor exactly (1, 0)); rows of
// `layer_row_stride` floats, ready for an in-place real-to-complex transform.
__global__ __launch_bounds__(256) void image_to_real_layer_kernel(
    float *__restrict__ layer, int64_t layer_row_stride, const float *__restrict__ image,
    int64_t image_row_stride, int G, const float *__restrict__ kernel1d, float lm_scale, float lm_bias)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= G)
        return;
    const int half = G / 2;
    const int sx = x < half ? x + half : x - half;
    const int sy = y < half ? y + half : y - half;
    const float l = lm_coord(x, lm_scale, lm_bias);
    const float m = lm_coord(y, lm_scale, lm_bias);
    const float l2 = l * l, m2 = m * m;
    const float n = sqrtf(1.0f - (m2 + l2));
    const float taper = kernel1d[y] * kernel1d[x];
    layer[(int64_t) sy * layer_row_stride + sx] = image[(int64_t) y * image_row_stride + x] / (taper * n);
}

// layer_to_grid from the half spectrum of a real layer: F(-k) = conj F(k).
__global__ __launch_bounds__(256) void half_layer_to_grid_kernel(
    float2 *__restrict__ grid, int64_t grid_row_stride, int Gg, const float2 *__restrict__ half_layer,
    int G)
{
    const int gx = blockIdx.x * blockDim.x + threadIdx.x;
    const int gy = blockIdx.y;
    if (gx >= Gg)
        return;
    const int half = Gg / 2, W = G / 2 + 1;
    int lx = gx - half, ly = gy - half;
    if (lx < 0) lx += G;
    if (ly < 0) ly += G;
    float2 v;
    if (lx < W) {
        v = half_layer[(int64_t) ly * W + lx];
    } else {
        v = half_layer[(int64_t) (ly ? G - ly : 0) * W + (G - lx)];
        v.y = -v.y;
    }
    grid[(int64_t) gy * grid_row_stride + gx] = v;
}

template <typename T> struct scale_t { T v[4]; };

template <typename T>
__global__ __launch_bounds__(256) void scale_kernel(
    T *__restrict__ image, int64_t row_stride, int64_t pol_stride, int width, int num_pols,
    scale_t<T> scale)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= width)
        return;
    int64_t addr = (int64_t) blockIdx.y * row_stride + x;
    for (int p = 0; p < num_pols; p++, addr += pol_stride)
        image[addr] *= scale.v[p];
}

// The same with the factors where an earlier kernel left them (kimg_pixel_reciprocal): a driver that
// scales by 1 / (a pixel of the image) need not read that pixel back first.
__global__ __launch_bounds__(256) void scale_device_kernel(
    float *__restrict__ image, int64_t row_stride, int64_t pol_stride, int width, int num_pols,
    const float *__restrict__ scale)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= width)
        return;
    int64_t addr = (int64_t) blockIdx.y * row_stride + x;
    for (int p = 0; p < num_pols; p++, addr += pol_stride)
        image[addr] *= scale[p];
}

__global__ void pixel_reciprocal_kernel(const float *__restrict__ image, int64_t pol_stride, int64_t offset,
                                        int num_pols, float *__restrict__ out)
{
    const int p = threadIdx.x;
    if (p < num_pols)
        out[p] = 1.0f / image[p * pol_stride + offset];     // (np.reciprocal of a float32: one rounding)
}

template <typename T>
__global__ __launch_bounds__(256) void add_image_kernel(
    T *__restrict__ dest, int64_t dest_row_stride, int64_t dest_pol_stride,
    const T *__restrict__ src, int64_t src_row_stride, int64_t src_pol_stride,
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

template <typename T>
__global__ __launch_bounds__(256) void apply_primary_beam_kernel(
    T *__restrict__ image, int64_t row_stride, int64_t pol_stride,
    const T *__restrict__ beam_power, int64_t beam_row_stride, int width, int num_pols,
    T threshold, T replacement)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= width)
        return;
    const T beam = beam_power[(int64_t) blockIdx.y * beam_row_stride + x];
    int64_t addr = (int64_t) blockIdx.y * row_stride + x;
    for (int p = 0; p < num_pols; p++, addr += pol_stride)
        image[addr] = beam < threshold ? replacement : image[addr] / beam;
}

// One thread per pixel of a row, one row of blocks per row: what every launch below but the
// reductions at the end of the file looks like.
template <typename... Params, typename... Args>
int launch_rows(void (*kernel)(Params...), int width, int height, void *stream, Args... args)
{
    kernel<<<dim3(kimg_divup(width, 256), height), 256, 0, (hipStream_t) stream>>>(args...);
    return kimg_launch_status();
}

// The checks and the launch of the operations that exist in both precisions: T = float behind the
// plain name, double behind *_f64 (the reference's --precision double; always the plain route:
// the own transforms of transform.hip and the w = 0 real route of this file are float32 only).
template <typename T>
int grid_to_layer_call(void *layer, int layer_size, const void *grid, int64_t grid_row_stride,
                       int grid_size, void *stream)
{
    KIMG_CHECK_ARG(layer && grid && layer_size > 0 && grid_size > 0 && grid_size <= layer_size);
    KIMG_CHECK_ARG(layer_size % 2 == 0 && grid_size % 2 == 0 && grid_row_stride >= grid_size);
    return launch_rows(grid_to_layer_kernel<T>, layer_size, layer_size, stream, (cplx<T> *) layer,
                       layer_size, (const cplx<T> *) grid, grid_row_stride, grid_size);
}

template <typename T>
int layer_to_grid_call(void *grid, int64_t grid_row_stride, int grid_size, const void *layer,
                       int layer_size, void *stream)
{
    KIMG_CHECK_ARG(layer && grid && layer_size > 0 && grid_size > 0 && grid_size <= layer_size);
    KIMG_CHECK_ARG(layer_size % 2 == 0 && grid_size % 2 == 0 && grid_row_stride >= grid_size);
    return launch_rows(layer_to_grid_kernel<T>, grid_size, grid_size, stream, (cplx<T> *) grid,
                       grid_row_stride, grid_size, (const cplx<T> *) layer, layer_size);
}

template <typename T>
int layer_to_image_call(T *image, int64_t image_row_stride, const void *layer, int size,
                        const T *kernel1d, T lm_scale, T lm_bias, T w, void *stream)
{
    KIMG_CHECK_ARG(image && layer && kernel1d && size > 0 && size % 2 == 0
                   && image_row_stride >= size);
    return launch_rows(layer_to_image_kernel<T>, size, size, stream, image, image_row_stride,
                       (const cplx<T> *) layer, size, kernel1d, lm_scale, lm_bias, w);
}

template <typename T>
int image_to_layer_call(void *layer, const T *image, int64_t image_row_stride, int size,
                        const T *kernel1d, T lm_scale, T lm_bias, T w, void *stream)
{
    KIMG_CHECK_ARG(image && layer && kernel1d && size > 0 && size % 2 == 0
                   && image_row_stride >= size);
    return launch_rows(image_to_layer_kernel<T>, size, size, stream, (cplx<T> *) layer, image,
                       image_row_stride, size, kernel1d, lm_scale, lm_bias, w);
}

// (P outside 1..4: KIMG_EUNSUPPORTED here, the factors travel in a scale_t; add_image and
// apply_primary_beam loop over P, refuse P <= 0 with KIMG_EINVAL and take any P above)
template <typename T>
int scale_call(T *image, int64_t row_stride, int64_t pol_stride, int width, int height,
               int num_polarizations, const T *scale_host, void *stream)
{
    KIMG_CHECK_ARG(image && scale_host && width > 0 && height > 0);
    KIMG_CHECK_ARG(row_stride >= width);
    if (num_polarizations < 1 || num_polarizations > 4)
        return KIMG_EUNSUPPORTED;
    scale_t<T> sc = {};
    for (int p = 0; p < num_polarizations; p++)
        sc.v[p] = scale_host[p];
    return launch_rows(scale_kernel<T>, width, height, stream, image, row_stride, pol_stride,
                       width, num_polarizations, sc);
}

template <typename T>
int add_image_call(T *dest, int64_t dest_row_stride, int64_t dest_pol_stride, const T *src,
                   int64_t src_row_stride, int64_t src_pol_stride, int width, int height,
                   int num_polarizations, void *stream)
{
    KIMG_CHECK_ARG(dest && src && width > 0 && height > 0 && num_polarizations > 0);
    KIMG_CHECK_ARG(dest_row_stride >= width && src_row_stride >= width);
    return launch_rows(add_image_kernel<T>, width, height, stream, dest, dest_row_stride,
                       dest_pol_stride, src, src_row_stride, src_pol_stride, width,
                       num_polarizations);
}

template <typename T>
int apply_primary_beam_call(T *image, int64_t row_stride, int64_t pol_stride, const T *beam_power,
                            int64_t beam_row_stride, int width, int height,
                            int num_polarizations, T threshold, T replacement, void *stream)
{
    KIMG_CHECK_ARG(image && beam_power && width > 0 && height > 0 && num_polarizations > 0);
    KIMG_CHECK_ARG(row_stride >= width && beam_row_stride >= width);
    return launch_rows(apply_primary_beam_kernel<T>, width, height, stream, image, row_stride,
                       pol_stride, beam_power, beam_row_stride, width, num_polarizations,
                       threshold, replacement);
}

} // namespace

extern "C" int kimg_grid_to_layer(void *layer, int layer_size, const void *grid,
                                  int64_t grid_row_stride, int grid_size, void *stream)
{
    return grid_to_layer_call<float>(layer, layer_size, grid, grid_row_stride, grid_size, stream);
}
extern "C" int kimg_grid_to_layer_f64(void *layer, int layer_size, const void *grid,
                                      int64_t grid_row_stride, int grid_size, void *stream)
{
    return grid_to_layer_call<double>(layer, layer_size, grid, grid_row_stride, grid_size, stream);
}

extern "C" int kimg_grid_to_half_layer(void *half_layer, int layer_size, const void *grid,
                                       int64_t grid_row_stride, int grid_size, void *stream)
{
    KIMG_CHECK_ARG(half_layer && grid && layer_size > 0 && layer_size % 2 == 0 && grid_size > 0
                   && grid_size % 2 == 0 && grid_size <= layer_size && grid_row_stride >= grid_size);
    return launch_rows(grid_to_half_layer_kernel, layer_size / 2 + 1, layer_size, stream,
                       static_cast<float2 *>(half_layer), layer_size,
                       static_cast<const float2 *>(grid), grid_row_stride, grid_size);
}

extern "C" int kimg_real_layer_to_image(float *image, int64_t image_row_stride, const float *layer,
                                        int64_t layer_row_stride, int size, const float *kernel1d,
                                        float lm_scale, float lm_bias, void *stream)
{
    KIMG_CHECK_ARG(image && layer && kernel1d && size > 0 && size % 2 == 0
                   && image_row_stride >= size && layer_row_stride >= size);
    return launch_rows(real_layer_to_image_kernel, size, size, stream, image, image_row_stride,
                       layer, layer_row_stride, size, kernel1d, lm_scale, lm_bias);
}

extern "C" int kimg_image_to_real_layer(float *layer, int64_t layer_row_stride, const float *image,
                                        int64_t image_row_stride, int size, const float *kernel1d,
                                        float lm_scale, float lm_bias, void *stream)
{
    KIMG_CHECK_ARG(image && layer && kernel1d && size > 0 && size % 2 == 0
                   && image_row_stride >= size && layer_row_stride >= size);
    return launch_rows(image_to_real_layer_kernel, size, size, stream, layer, layer_row_stride,
                       image, image_row_stride, size, kernel1d, lm_scale, lm_bias);
}

extern "C" int kimg_half_layer_to_grid(void *grid, int64_t grid_row_stride, int grid_size,
                                       const void *half_layer, int layer_size, void *stream)
{
    KIMG_CHECK_ARG(half_layer && grid && layer_size > 0 && layer_size % 2 == 0 && grid_size > 0
                   && grid_size % 2 == 0 && grid_size <= layer_size && grid_row_stride >= grid_size);
    return launch_rows(half_layer_to_grid_kernel, grid_size, grid_size, stream,
                       static_cast<float2 *>(grid), grid_row_stride, grid_size,
                       static_cast<const float2 *>(half_layer), layer_size);
}

extern "C" int kimg_layer_to_grid(void *grid, int64_t grid_row_stride, int grid_size,
                                  const void *layer, int layer_size, void *stream)
{
    return layer_to_grid_call<float>(grid, grid_row_stride, grid_size, layer, layer_size, stream);
}
extern "C" int kimg_layer_to_grid_f64(void *grid, int64_t grid_row_stride, int grid_size,
                                      const void *layer, int layer_size, void *stream)
{
    return layer_to_grid_call<double>(grid, grid_row_stride, grid_size, layer, layer_size, stream);
}

extern "C" int kimg_layer_to_image(float *image, int64_t image_row_stride, const void *layer,
                                   int size, const float *kernel1d, float lm_scale,
                                   float lm_bias, float w, void *stream)
{
    return layer_to_image_call<float>(image, image_row_stride, layer, size, kernel1d, lm_scale,
                                      lm_bias, w, stream);
}
extern "C" int kimg_layer_to_image_f64(double *image, int64_t image_row_stride, const void *layer,
                                       int size, const double *kernel1d, double lm_scale,
                                       double lm_bias, double w, void *stream)
{
    return layer_to_image_call<double>(image, image_row_stride, layer, size, kernel1d, lm_scale,
                                       lm_bias, w, stream);
}

extern "C" int kimg_image_to_layer(void *layer, const float *image, int64_t image_row_stride,
                                   int size, const float *kernel1d, float lm_scale,
                                   float lm_bias, float w, void *stream)
{
    return image_to_layer_call<float>(layer, image, image_row_stride, size, kernel1d, lm_scale,
                                      lm_bias, w, stream);
}
extern "C" int kimg_image_to_layer_f64(void *layer, const double *image, int64_t image_row_stride,
                                       int size, const double *kernel1d, double lm_scale,
                                       double lm_bias, double w, void *stream)
{
    return image_to_layer_call<double>(layer, image, image_row_stride, size, kernel1d, lm_scale,
                                       lm_bias, w, stream);
}

extern "C" int kimg_scale(float *image, int64_t row_stride, int64_t pol_stride, int width,
                          int height, int num_polarizations, const float *scale_host, void *stream)
{
    return scale_call<float>(image, row_stride, pol_stride, width, height, num_polarizations,
                             scale_host, stream);
}
extern "C" int kimg_scale_f64(double *image, int64_t row_stride, int64_t pol_stride, int width,
                              int height, int num_polarizations, const double *scale_host,
                              void *stream)
{
    return scale_call<double>(image, row_stride, pol_stride, width, height, num_polarizations,
                              scale_host, stream);
}

extern "C" int kimg_pixel_reciprocal(const float *image, int64_t row_stride, int64_t pol_stride,
                                     int width, int height, int num_polarizations, int x, int y,
                                     float *out, void *stream)
{
    KIMG_CHECK_ARG(image && out && x >= 0 && x < width && y >= 0 && y < height);
    KIMG_CHECK_ARG(row_stride >= width);
    if (num_polarizations < 1 || num_polarizations > 4)
        return KIMG_EUNSUPPORTED;
    pixel_reciprocal_kernel<<<1, 64, 0, (hipStream_t) stream>>>(image, pol_stride, (int64_t) y * row_stride + x,
                                                                num_polarizations, out);
    return kimg_launch_status();
}

extern "C" int kimg_scale_device(float *image, int64_t row_stride, int64_t pol_stride, int width,
                                 int height, int num_polarizations, const float *scale, void *stream)
{
    KIMG_CHECK_ARG(image && scale && width > 0 && height > 0);
    KIMG_CHECK_ARG(row_stride >= width);
    if (num_polarizations < 1 || num_polarizations > 4)
        return KIMG_EUNSUPPORTED;
    return launch_rows(scale_device_kernel, width, height, stream, image, row_stride, pol_stride,
                       width, num_polarizations, scale);
}

extern "C" int kimg_add_image(float *dest, int64_t dest_row_stride, int64_t dest_pol_stride,
                              const float *src, int64_t src_row_stride, int64_t src_pol_stride,
                              int width, int height, int num_polarizations, void *stream)
{
    return add_image_call<float>(dest, dest_row_stride, dest_pol_stride, src, src_row_stride,
                                 src_pol_stride, width, height, num_polarizations, stream);
}
extern "C" int kimg_add_image_f64(double *dest, int64_t dest_row_stride, int64_t dest_pol_stride,
                                  const double *src, int64_t src_row_stride,
                                  int64_t src_pol_stride, int width, int height,
                                  int num_polarizations, void *stream)
{
    return add_image_call<double>(dest, dest_row_stride, dest_pol_stride, src, src_row_stride,
                                  src_pol_stride, width, height, num_polarizations, stream);
}

extern "C" int kimg_apply_primary_beam(float *image, int64_t row_stride, int64_t pol_stride,
                                       const float *beam_power, int64_t beam_row_stride,
                                       int width, int height, int num_polarizations,
                                       float threshold, float replacement, void *stream)
{
    return apply_primary_beam_call<float>(image, row_stride, pol_stride, beam_power,
                                          beam_row_stride, width, height, num_polarizations,
                                          threshold, replacement, stream);
}
extern "C" int kimg_apply_primary_beam_f64(double *image, int64_t row_stride, int64_t pol_stride,
                                           const double *beam_power, int64_t beam_row_stride,
                                           int width, int height, int num_polarizations,
                                           double threshold, double replacement, void *stream)
{
    return apply_primary_beam_call<double>(image, row_stride, pol_stride, beam_power,
                                           beam_row_stride, width, height, num_polarizations,
                                           threshold, replacement, stream);
}

// ---- restoring beam in the Fourier domain: beam.py:283-311 + fourier_beam.mako ----------
namespace {
__global__ __launch_bounds__(256) void fourier_beam_kernel(
    float2 *__restrict__ data, int64_t stride, float amplitude, float a, float b, float c,
    int width, int height)
{
    int x = blockIdx.x * blockDim.x + threadIdx.x;
    int y = blockIdx.y;
    if (x >= width)
        return;
    float u = (float) x;                 // only the non-negative half of this axis is stored
    float v = (float) ((y * 2 >= height) ? y - height : y);
    float power = (a * v + b * u) * v + c * u * u;
    float ft = amplitude * expf(power);
    int64_t addr = (int64_t) y * stride + x;
    float2 value = data[addr];
    value.x *= ft;
    value.y *= ft;
    data[addr] = value;
}
}  // namespace

extern "C" int kimg_fourier_beam(void *data, int64_t row_stride, int width, int height,
                                 float amplitude, float a, float b, float c, void *stream)
{
    KIMG_CHECK_ARG(width >= 0 && height >= 0 && row_stride >= width);
    if (width == 0 || height == 0)
        return 0;
    KIMG_CHECK_ARG(data != nullptr && height <= 65535);
    return launch_rows(fourier_beam_kernel, width, height, stream, static_cast<float2 *>(data),
                       row_stride, amplitude, a, b, c, width, height);
}

// ---- output statistics of the restore step: frontend.py:171-209 -------------------------------
namespace {
// find_peak (frontend.py:171-194): max |image| over pixels with |image| * pbeam > 7.5 noise
// (comparisons with NaN are false, as on the host).  |x| >= 0, so the float maximum is the
// maximum of the bit patterns.
__global__ __launch_bounds__(256) void image_peak_kernel(
    const float *__restrict__ image, int64_t row_stride, int64_t pol_stride,
    const float *__restrict__ pbeam, int64_t beam_row_stride, int width, int height, int P,
    float limit, unsigned int *__restrict__ out)
{
    float peak = 0.0f;
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    constexpr int ROWS = 4;     // rows in flight per thread
    if (x < width)
        for (int y0 = blockIdx.y; y0 < height; y0 += gridDim.y * ROWS)
            for (int p = 0; p < P; p++) {
                float v[ROWS], pb[ROWS];
#pragma unroll
                for (int r = 0; r < ROWS; r++) {
                    const int y = y0 + r * gridDim.y;
                    const bool ok = y < height;
                    v[r] = ok ? fabsf(image[p * pol_stride + (int64_t) y * row_stride + x]) : 0.0f;
                    pb[r] = (ok && pbeam) ? pbeam[(int64_t) y * beam_row_stride + x] : 1.0f;
                }
#pragma unroll
                for (int r = 0; r < ROWS; r++)
                    if (v[r] > peak && v[r] * pb[r] > limit)
                        peak = v[r];
            }
    peak = fmaxf(peak, __shfl_xor(peak, 32, WAVE));
#pragma unroll
    for (int off = 16; off > 0; off >>= 1)
        peak = fmaxf(peak, __shfl_xor(peak, off, WAVE));
    // one atomic per workgroup (atomics on one address are served one after the other)
    __shared__ float part[4];
    if ((threadIdx.x & 63) == 0)
        part[threadIdx.x >> 6] = peak;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int) (blockDim.x >> 6); w++)
            peak = fmaxf(peak, part[w]);
        if (peak > 0.0f)
            atomicMax(out, __float_as_uint(peak));
    }
}

// get_totals (frontend.py:197-209): per-polarization sum ignoring NaNs, in float64.
__global__ __launch_bounds__(256) void image_nansum_kernel(
    const float *__restrict__ image, int64_t row_stride, int64_t pol_stride, int width,
    int height, double *__restrict__ sums)
{
    const int p = blockIdx.z;
    double acc = 0.0;
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    constexpr int ROWS = 4;
    if (x < width)
        for (int y0 = blockIdx.y; y0 < height; y0 += gridDim.y * ROWS) {
            float v[ROWS];
#pragma unroll
            for (int r = 0; r < ROWS; r++) {
                const int y = y0 + r * gridDim.y;
                v[r] = y < height ? image[p * pol_stride + (int64_t) y * row_stride + x] : 0.0f;
            }
#pragma unroll
            for (int r = 0; r < ROWS; r++)
                if (v[r] == v[r])
                    acc += (double) v[r];
        }
    acc = wave_sum(acc);
    __shared__ double part[4];
    if ((threadIdx.x & 63) == 0)
        part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < (int) (blockDim.x >> 6); w++)
            t += part[w];
        atomicAdd(&sums[p], t);
    }
}
}  // namespace

extern "C" int kimg_image_peak(const float *image, int64_t row_stride, int64_t pol_stride,
                               const float *pbeam, int64_t beam_row_stride, int width, int height,
                               int num_polarizations, float noise, float *peak, void *stream)
{
    KIMG_CHECK_ARG(image && peak && width > 0 && height > 0 && num_polarizations >= 1);
    KIMG_CHECK_ARG(row_stride >= width && (pbeam == nullptr || beam_row_stride >= width));
    hipStream_t s = (hipStream_t) stream;
    KIMG_HIP(hipMemsetAsync(peak, 0, sizeof(float), s));
    int by = height < 64 ? height : 64;
    dim3 grid(kimg_divup(width, 256), by);
    image_peak_kernel<<<grid, 256, 0, s>>>(image, row_stride, pol_stride, pbeam, beam_row_stride,
                                           width, height, num_polarizations, 7.5f * noise,
                                           reinterpret_cast<unsigned int *>(peak));
    return kimg_launch_status();
}

extern "C" int kimg_image_nansum(const float *image, int64_t row_stride, int64_t pol_stride,
                                 int width, int height, int num_polarizations, double *sums,
                                 void *stream)
{
    KIMG_CHECK_ARG(image && sums && width > 0 && height > 0 && num_polarizations >= 1
                   && num_polarizations <= 65535);
    KIMG_CHECK_ARG(row_stride >= width);
    hipStream_t s = (hipStream_t) stream;
    KIMG_HIP(hipMemsetAsync(sums, 0, sizeof(double) * num_polarizations, s));
    int by = height < 32 ? height : 32;
    dim3 grid(kimg_divup(width, 256), by, num_polarizations);
    image_nansum_kernel<<<grid, 256, 0, s>>>(image, row_stride, pol_stride, width, height, sums);
    return kimg_launch_status();
}

// (kimg_preload, api.hip)
KIMG_PRELOAD_THIS_UNIT(grid_to_half_layer_kernel)
