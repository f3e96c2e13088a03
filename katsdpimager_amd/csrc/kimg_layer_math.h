// Per-pixel arithmetic that the layer kernels (image.hip) and the library's own transforms
// (transform.hip) share: both must round exactly alike, so it is written once.
#pragma once
#include "kimg_common.h"

namespace {

__device__ inline float real_rint(float x) { return rintf(x); }
__device__ inline double real_rint(double x) { return rint(x); }
__device__ inline float real_sqrt(float x) { return sqrtf(x); }
__device__ inline double real_sqrt(double x) { return sqrt(x); }
__device__ inline void real_sincospi(float x, float *s, float *c) { sincospif(x, s, c); }
__device__ inline void real_sincospi(double x, double *s, double *c) { sincospi(x, s, c); }

// A transform that is only wanted for its REAL part (the W-stack phase is 1 at
// w = 0): Re F^-1[g] = F^-1[h] with h(k) = (g(k) + conj g(-k)) / 2, and h is Hermitian, so half
// of it -- columns 0 .. G/2 -- feeds a complex-to-real transform of half the size (the
// "opportunity" noted at image.py:561-566 of the reference).  half[ly][lx], row length G/2 + 1.
__device__ inline float2 half_layer_value(const float2 *__restrict__ grid, int64_t grid_row_stride,
                                          int Gg, int G, int lx, int ly)
{
    const int half = Gg / 2;
    const int cx = lx < G - half ? lx : lx - G;
    const int cy = ly < G - half ? ly : ly - G;
    float2 a = make_float2(0.0f, 0.0f), b = make_float2(0.0f, 0.0f);
    if (cx >= -half && cx < half && cy >= -half && cy < half)
        a = grid[(int64_t) (cy + half) * grid_row_stride + (cx + half)];
    // -k modulo G: the Nyquist row and column (a grid as large as the layer has them) are their
    // own mirrors
    const int mlx = lx ? G - lx : 0, mly = ly ? G - ly : 0;
    const int mx = mlx < G - half ? mlx : mlx - G;
    const int my = mly < G - half ? mly : mly - G;
    if (mx >= -half && mx < half && my >= -half && my < half)
        b = grid[(int64_t) (my + half) * grid_row_stride + (mx + half)];
    return make_float2(0.5f * (a.x + b.x), 0.5f * (a.y - b.y));
}

// e^{2 pi i x} with the reference's range reduction (fast_math.py:14-15).
template <typename T>
__device__ inline void expj2pi(T x, T &c, T &s)
{
    T r = x - real_rint(x);
    real_sincospi(T(2) * r, &s, &c);
}

// n(l, m) following GridToImageHost.__call__ (image.py:785-790) operation by operation.
template <typename T>
__device__ inline T lm_coord(int i, T lm_scale, T lm_bias)
{
    return (T) i * lm_scale + lm_bias;
}

} // namespace
