"""Every strided entry point of include/kimg.h on padded, offset and non-square layouts.

The Python wrappers only ever pass dense layouts (row_stride = W, pol_stride = H * W).  Here every
call goes through the C ABI with raw pointers into helpers.Padded buffers: odd row padding (3 or 7
elements, so rows lose 8- and 16-byte alignment), 2 extra rows per polarization plane, and in one
layout per call an interior that starts at row 1, column 1 of the buffer (a sub-image pointer that
is only element-aligned).  Two strided arrays of one call get different paddings.  Padding is a
huge finite value (a mask's: 1 = allowed), so a kernel that indexes with `width` where it means
`row_stride`, or with `height * row_stride` where it means `pol_stride`, reads or writes it:
Padded.get asserts that no padding byte changed, and every interior is compared with an
independent expectation (numpy, math.fsum, oracle/), never with a dense run of the same kernel.

Shapes: H = 300, W = 302 (two x-blocks of 256 with a 46-wide tail; the row loops of image_peak,
by = 64, and image_nansum, by = 32, wrap with a ragged last group of 4 rows; H != W, both even as
kimg_grid_weights needs) and H = 6, W = 10, P = 3 (height < by); mean weight and density weights
also at H = 500, W = 2100 (image_grid of weight.hip: bx = 9, by = 113, a second, ragged round).
The layer copies and CLEAN are square by contract.

Alignment kept on purpose where include/kimg.h states one: kimg_fill's data pointer (16 bytes).

entry point                           test
------------------------------------  ----------------------------------------
kimg_scale, kimg_scale_f64            test_scale
kimg_scale_device                     test_scale
kimg_pixel_reciprocal                 test_scale
kimg_add_image, kimg_add_image_f64    test_add_image
kimg_apply_primary_beam (+ _f64)      test_apply_primary_beam
kimg_fill                             test_fill
kimg_real_to_complex                  test_real_to_complex
kimg_image_peak                       test_image_peak
kimg_image_nansum                     test_image_nansum
kimg_psf_patch                        test_psf_patch
kimg_abs_histogram                    test_noise_selection
kimg_abs_count_le                     test_noise_selection
kimg_noise_est                        test_noise_selection
kimg_grid_weights                     test_grid_weights
kimg_mean_weight                      test_density_weights
kimg_density_weights                  test_density_weights
kimg_density_weights_robust           test_density_weights
kimg_grid_to_layer (+ _f64)           test_layer_copies
kimg_layer_to_grid (+ _f64)           test_layer_copies
kimg_grid_to_half_layer               test_half_layer_copies
kimg_half_layer_to_grid               test_half_layer_copies
kimg_layer_to_image (+ _f64)          test_layer_image
kimg_image_to_layer (+ _f64)          test_layer_image
kimg_real_layer_to_image              test_real_layer_image
kimg_image_to_real_layer              test_real_layer_image
kimg_fourier_beam                     test_fourier_beam
kimg_update_tiles (+ _masked)         test_clean_steps, test_clean_loops
kimg_find_peak (+ _masked)            test_clean_steps
kimg_subtract_psf                     test_clean_steps
kimg_clean_cycles (+ _masked)         test_clean_loops
kimg_clean_major_cycles               test_clean_loops
kimg_clean_cycles_batch               test_clean_loops
kimg_grid, kimg_grid_f64              test_gridders
kimg_degrid, kimg_degrid_f64          test_degridders
kimg_grid_to_image_real / _w          test_routes
kimg_image_to_grid_real / _w          test_routes
kimg_convolve_beam                    test_convolve_beam
every call with a row stride          test_stride_below_width_is_refused (and, stride = width
                                      accepted: the CPU test)
"""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import test_exact_gridding as eg                # noqa: E402
import test_transform_truth as tt               # noqa: E402
from helpers import Padded, context_queue, grid_to_image_truth      # noqa: E402
from oracle import kimg_oracle as orc           # noqa: E402

gpu = pytest.mark.gpu
KIMG_EINVAL = -10001

# (first array's layout, second array's layout): odd row paddings, 2 extra rows, one origin (1, 1)
LAYOUTS = {
    'r3': (dict(rpad=3, vpad=2, origin=(0, 0)), dict(rpad=7, vpad=2, origin=(1, 1))),
    'r7_origin': (dict(rpad=7, vpad=2, origin=(1, 1)), dict(rpad=3, vpad=2, origin=(0, 0))),
}
SHAPES = [(300, 302, 1), (300, 302, 3), (300, 302, 4), (6, 10, 3), (6, 10, 2)]

layouts = pytest.mark.parametrize('layout', list(LAYOUTS))
shapes = pytest.mark.parametrize('H,W,P', SHAPES)


# ---------------------------------------------------------------------------------------------
# expectations (numpy / math.fsum / oracle; the CPU test below runs them on dense inputs)

def fsum_bound(values):
    """Absolute bound on a float64 sum of `values` taken in any order: n * 2^-52 * fsum(|x|)
    (the first-order bound (n - 1) 2^-53 sum |x| of recursive summation in any order, doubled)."""
    values = np.asarray(values, np.float64).ravel()
    return len(values) * 2.0 ** -52 * math.fsum(np.abs(values))


def expect_nansum(image):
    """(per-polarization fsum of the non-NaN pixels, its bound)."""
    sums, bounds = [], []
    for plane in image:
        x = plane[~np.isnan(plane)].astype(np.float64)
        finite = x[np.isfinite(x)]
        if len(finite) < len(x):        # an infinity decides the sum
            sums.append(float(np.sum(x[~np.isfinite(x)])))
            bounds.append(0.0)
        else:
            sums.append(math.fsum(x))
            bounds.append(fsum_bound(x))
    return np.array(sums), np.array(bounds)


def expect_primary_beam(image, beam, threshold, replacement):
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(beam < threshold, image.dtype.type(replacement), image / beam)


def expect_histogram(image, border, pass_, prefix):
    P, H, W = image.shape
    bits = np.abs(image[:, border:H - border, border:W - border]).view(np.uint32).astype(np.uint64).ravel()
    take = (bits >> np.uint64(8 * (pass_ + 1))) == np.uint64(prefix)
    return np.bincount(((bits[take] >> np.uint64(8 * pass_)) & np.uint64(255)).astype(np.int64),
                       minlength=256).astype(np.uint32)


def expect_count_le(image, border, value):
    P, H, W = image.shape
    a = np.abs(image[:, border:H - border, border:W - border]).ravel()
    above = a[a > value]
    nxt = above.min().view(np.uint32) if len(above) else np.uint32(0xffffffff)
    return np.array([np.count_nonzero(a <= value), nxt], np.uint32)


def expect_noise(image, border):
    P, H, W = image.shape
    inner = np.abs(image[:, border:H - border, border:W - border])
    return np.float32(np.median(inner) * np.float32(orc.MEDIAN_TO_RMS))


def expect_density(weights, a, b):
    """The kernel's float32 steps (no contraction, correctly rounded division): d and the three
    sums over polarization 0 with their bounds."""
    w = np.asarray(weights, np.float32)
    with np.errstate(divide='ignore'):
        d = np.where(w != 0, np.float32(1) / (np.float32(a) * w + np.float32(b)), np.float32(0)).astype(np.float32)
    w0, d0 = w[0].astype(np.float64).ravel(), d[0].astype(np.float64).ravel()
    terms = (w0, d0 * w0, d0 * (d0 * w0))
    return d, np.array([math.fsum(t) for t in terms]), np.array([fsum_bound(t) for t in terms])


def expect_grid_to_layer(grid, G):
    Gg = grid.shape[0]
    big = np.zeros((G, G), grid.dtype)
    big[G // 2 - Gg // 2:G // 2 + Gg // 2, G // 2 - Gg // 2:G // 2 + Gg // 2] = grid
    return np.fft.ifftshift(big)


def expect_layer_to_grid(layer, Gg):
    G = layer.shape[0]
    return np.fft.fftshift(layer)[G // 2 - Gg // 2:G // 2 + Gg // 2, G // 2 - Gg // 2:G // 2 + Gg // 2]


def mirror(layer):
    """layer[-k] (indices modulo the size)."""
    return np.roll(layer[::-1, ::-1], 1, axis=(0, 1))


def expect_half_layer(grid, G):
    full = expect_grid_to_layer(grid, G)
    herm = (full + np.conj(mirror(full))) * np.complex64(0.5)
    return herm[:, :G // 2 + 1]


def expect_half_layer_to_grid(half, Gg):
    G = half.shape[0]
    full = np.zeros((G, G), np.complex64)
    full[:, :G // 2 + 1] = half
    m = np.conj(mirror(full))
    full[:, G // 2 + 1:] = m[:, G // 2 + 1:]
    return expect_layer_to_grid(full, Gg)


def correction(G, k1d, lm_scale, lm_bias, w, dtype):
    """n, t, reduced phase r (turns) in the arithmetic of `dtype`, step by step as include/kimg.h
    gives them (tests/test_transform_truth.py: correction32)."""
    f = np.dtype(dtype).type
    lm = np.arange(G).astype(dtype) * f(lm_scale) + f(lm_bias)
    l2 = lm * lm
    n = np.sqrt(f(1) - (l2[:, None] + l2[None, :]))
    k = np.asarray(k1d, dtype)
    p = f(w) * (n - f(1))
    return n, k[:, None] * k[None, :], p - np.rint(p)


# The truths of the layer <-> image kernels are evaluated in extended precision: a float64 truth
# carries about as much rounding as the float64 kernels it is to judge.
WIDE = np.longdouble
WIDE_PI = 4 * np.arctan(WIDE(1))
assert np.finfo(WIDE).eps <= 2.0 ** -63, 'these truths need a long double wider than float64'


def expect_layer_to_image(prefill, layer, k1d, lm_scale, lm_bias, w):
    """(extended-precision value, bound).  The kernel's n, t and reduced phase are reproduced step
    by step in its own arithmetic (eps = 2^-24 or 2^-53); what is left is what the module docstring
    of tests/test_transform_truth.py bounds for the same steps, with its constants: the rotation by
    cos / sin of the exactly reduced phase (each within DELTA = 4 u, the ceiling OpenCL sets for
    sincospi), two products and a subtraction: ROT = 8 u of |layer cell|; times n and over t: 2 u;
    the final += : u |result|.  For float64 the constants scale with eps / u."""
    real = prefill.dtype
    eps = np.finfo(real).eps / 2
    n, t, r = correction(len(k1d), k1d, lm_scale, lm_bias, w, real)
    n, t, r = (z.astype(WIDE) for z in (n, t, r))
    v = np.fft.fftshift(layer)
    re, im = v.real.astype(WIDE), v.imag.astype(WIDE)
    rotated = re * np.cos(2 * WIDE_PI * r) - im * np.sin(2 * WIDE_PI * r)
    want = prefill.astype(WIDE) + rotated * n / t
    k = eps / tt.U
    bound = k * (tt.ROT + 2 * tt.U) * np.hypot(re, im) * n / t + eps * np.abs(want)
    return want, bound


def expect_image_to_layer(image, k1d, lm_scale, lm_bias, w):
    """(extended-precision layer, bound): v = image / (t n) in the kernel's arithmetic exactly; the phase
    factor is within DELTA = 4 u per component (tests/test_transform_truth.py, as above) and the
    product rounds once: (DELTA + u) |v| per component, scaled by eps / u for float64."""
    real = image.dtype
    eps = np.finfo(real).eps / 2
    n, t, r = correction(len(k1d), k1d, lm_scale, lm_bias, -w, real)
    v = (image / (t * n)).astype(WIDE)
    r = r.astype(WIDE)
    layer = v * np.cos(2 * WIDE_PI * r) + 1j * (v * np.sin(2 * WIDE_PI * r))
    return np.fft.ifftshift(layer), np.fft.ifftshift(eps / tt.U * (tt.DELTA + tt.U) * np.abs(v))


def expect_fourier_beam(data, amplitude, a, b, c):
    """float32 steps of the kernel's power, reproduced exactly; the rest as the module docstring of
    tests/test_transform_truth.py has it for the same factor: expf within 2 ulp, one product with
    the amplitude, one with the cell: 6 u |result| per component."""
    H, W = data.shape
    y = np.arange(H)
    v = np.where(2 * y >= H, y - H, y).astype(np.float32)[:, None]
    u = np.arange(W, dtype=np.float32)[None, :]
    a, b, c = np.float32(a), np.float32(b), np.float32(c)
    power = (a * v + b * u) * v + c * u * u
    ft = float(np.float32(amplitude)) * np.exp(power.astype(np.float64))
    want = data.astype(np.complex128) * ft
    return want, 6 * tt.U * np.abs(want)


def embed(grid, G):
    """The centred Gg x Gg grid in a G x G grid of zeros, as [1][G][G] complex128."""
    Gg = grid.shape[0]
    big = np.zeros((1, G, G), np.complex128)
    big[0, G // 2 - Gg // 2:G // 2 + Gg // 2, G // 2 - Gg // 2:G // 2 + Gg // 2] = grid
    return big


def expect_grid_to_image(op, grid, G, k1d, lm_scale, lm_bias, w, prefill=None):
    """(helpers.grid_to_image_truth of the embedded grid, the norm-wise allowance of
    tests/test_transform_truth.py for `op` at this size, n / t).  The allowance is that module's:
    ||(got - truth) t / n||_F <= transform_bound(op, G, True) ||F||_F (F the transform itself;
    its real part for the w = 0 route), plus, accumulating, u (|old| + |out|) (its docstring)."""
    big = embed(grid, G)
    truth = grid_to_image_truth(big, k1d, lm_scale, lm_bias, w)[0]
    F = np.fft.fftshift(np.fft.ifft2(np.fft.ifftshift(big[0]))) * (G * G)
    n, t, _ = correction(G, k1d, lm_scale, lm_bias, 0.0, np.float32)
    corr = n.astype(np.float64) / t.astype(np.float64)
    allowed = tt.transform_bound(op, G, True) * np.linalg.norm(F if op == 'g2i_w' else F.real)
    if prefill is not None:
        allowed += tt.U * np.linalg.norm((np.abs(prefill) + np.abs(truth)) / corr)
        truth = truth + prefill
    return truth, allowed, corr


def expect_image_to_grid(op, image, Gg, k1d, lm_scale, lm_bias, w):
    """(the float64 orc.image_to_grid, centre Gg x Gg; the module's norm-wise allowance
    transform_bound(op, G, True) G ||image / (t n)||_F)."""
    G = image.shape[0]
    full, _ = orc.image_to_grid(image[np.newaxis].astype(np.float64), np.asarray(k1d, np.float64),
                                float(lm_scale), float(lm_bias), float(w), np.complex128)
    n, t, _ = correction(G, k1d, lm_scale, lm_bias, 0.0, np.float32)
    mag = image.astype(np.float64) / (t.astype(np.float64) * n.astype(np.float64))
    allowed = tt.transform_bound(op, G, True) * G * np.linalg.norm(mag)
    return expect_layer_to_grid(np.fft.ifftshift(full[0]), Gg), allowed


BEAM = (1.3, 2.2, 3.7, 0.6)         # amplitude, standard deviations, angle


def expect_convolve_beam(model):
    """(orc.convolve_beam in float64, the coefficients of the call, the module's norm-wise allowance
    transform_bound('beam', G, True) Bmax G^2 ||x||_F with the 1 / G^2 inside Bmax)."""
    G = model.shape[0]
    coeff = tt.beam_coefficients(G, *BEAM)
    truth = orc.convolve_beam(model[np.newaxis].astype(np.float64), *BEAM)[0]
    bmax = float(tt.beam_factor(G, *coeff).max())
    return truth, coeff, tt.transform_bound('beam', G, True) * bmax * G * G * np.linalg.norm(model.astype(np.float64))


def weights_stream(H, W, P, seed):
    """(uv int16 [N + 64][4], weights float32 [N + 64][P], N): integer weights up to 64 (float32
    atomic addition is then exact in any order); runs of equal (u, v) across a 64-lane and a
    256-thread boundary and one ending exactly at N - 1 with N % 64 != 0; negative u with
    non-negative v and the reverse (the packed 4-byte key); the four corner cells; garbage
    beyond N."""
    rs = np.random.RandomState(seed)
    N = 64 * 9 + 37
    u = rs.randint(-W // 2, W // 2, N)
    v = rs.randint(-H // 2, H // 2, N)
    u[40:75], v[40:75] = -2, 1                  # crosses lane 64 (negative u, non-negative v)
    u[250:262], v[250:262] = 2, -1              # crosses thread 256 (the reverse)
    u[N - 5:], v[N - 5:] = W // 2 - 1, H // 2 - 1       # ends at N - 1, the last row and column
    u[300:304] = [-W // 2, W // 2 - 1, -W // 2, 0]
    v[300:304] = [-H // 2, -H // 2, H // 2 - 1, -H // 2]
    uv = rs.randint(-30000, 30000, (N + 64, 4)).astype(np.int16)
    uv[:N, 0], uv[:N, 1] = u, v
    weights = rs.randint(1, 65, (N + 64, P)).astype(np.float32)
    weights[N:] = 1e30
    assert N % 64 != 0
    return uv, weights, N


def expect_grid_weights(prefill, uv, weights, N):
    want = prefill.copy()
    orc.weights_grid_add(want, uv[:N], weights[:N])
    return want


def test_padded_helper_and_expectations_on_the_cpu():
    """Padded without a device: build-up, interior view, strides, pointer offset, detection of one
    changed padding byte; and the expectation functions above on small dense inputs with known
    answers (a broken truth fails here, without a GPU)."""
    rs = np.random.RandomState(0)
    for dtype in (np.float32, np.float64, np.complex64, np.complex128, np.uint8):
        inner = (rs.uniform(1, 100, (3, 5, 7))).astype(dtype)
        p = Padded(None, None, inner, rpad=3, vpad=2, origin=(1, 2))
        assert p.row == 2 + 7 + 3 and p.pol == (1 + 5 + 2) * p.row
        assert p.ptr - p.dev.ptr == (1 * p.row + 2) * np.dtype(dtype).itemsize
        np.testing.assert_array_equal(p.get(), inner)
        flat = p.dev.get().reshape(-1)
        for pol in range(3):
            for y in range(5):
                at = p.offset + pol * p.pol + y * p.row
                np.testing.assert_array_equal(flat[at:at + 7], inner[pol, y])
        assert np.count_nonzero(p.host != p.host[0, 0, 0]) <= inner.size
        # one padding byte changed in the buffer (each side of the interior in turn)
        for where in (0, p.offset - 1, p.offset + 7, p.host.size - 1):
            q = Padded(None, None, inner, rpad=3, vpad=2, origin=(1, 2))
            q.dev.tensor[where * np.dtype(dtype).itemsize] ^= 0x10
            with pytest.raises(AssertionError, match='padding changed'):
                q.get()
        # ... while a changed interior is handed back, not refused
        q = Padded(None, None, inner, rpad=3, vpad=2, origin=(1, 2))
        q.dev.tensor[q.offset * np.dtype(dtype).itemsize] ^= 0x01
        assert np.count_nonzero(q.get() != inner) == 1
    plane = Padded(None, None, np.arange(12, dtype=np.uint8).reshape(3, 4), rpad=5)
    assert plane.row == 9 and plane.get().shape == (3, 4) and plane.host[0, 0, 4] == 1
    old = Padded(None, None, np.zeros((2, 4, 4), np.complex64), 7, 3, np.complex64(3e6 - 5e6j))
    assert (old.row, old.pol, old.ptr) == (11, 77, old.dev.ptr)

    # expectations on known answers
    x = np.array([[[1.0, np.nan], [2.5, -4.0]], [[np.inf, 1.0], [np.nan, 2.0]]], np.float32)
    sums, bounds = expect_nansum(x)
    assert sums[0] == -0.5 and sums[1] == np.inf and bounds[0] == 3 * 2.0 ** -52 * 7.5
    assert fsum_bound([1.0, -2.0]) == 2 * 2.0 ** -52 * 3.0
    img = np.array([[[1.0, 2.0, 3.0]]], np.float32)
    beam = np.array([[0.1, 0.25, 0.5]], np.float32)
    np.testing.assert_array_equal(expect_primary_beam(img, beam, 0.25, 9.0), [[[9.0, 8.0, 6.0]]])
    h = expect_histogram(np.array([[[1.0, -1.0, 2.0, 0.0]]], np.float32), 0, 3, 0)
    assert h[0x3f] == 2 and h[0x40] == 1 and h[0] == 1 and h.sum() == 4
    h = expect_histogram(np.array([[[1.0, -1.5, 2.0, 0.0]]], np.float32), 0, 2, 0x3f)
    assert h[0x80] == 1 and h[0xc0] == 1 and h.sum() == 2
    c = expect_count_le(np.array([[[1.0, -1.5, 2.0, 0.0]]], np.float32), 0, np.float32(1.0))
    assert c[0] == 2 and c[1] == np.float32(1.5).view(np.uint32)
    assert expect_count_le(np.ones((1, 1, 3), np.float32), 0, np.float32(1.0))[1] == 0xffffffff
    assert expect_noise(np.array([[[9, 9, 9, 9], [9, 1, -3, 9], [9, 9, 9, 9]]], np.float32).reshape(1, 3, 4), 1) \
        == np.float32(2.0) * np.float32(orc.MEDIAN_TO_RMS)
    d, s, _ = expect_density(np.array([[[0.0, 1.0, 3.0]]], np.float32), 2.0, 2.0)
    np.testing.assert_array_equal(d, [[[0.0, 0.25, 0.125]]])
    np.testing.assert_array_equal(s, [4.0, 0.25 + 0.375, 0.0625 + 3 / 64])
    g = np.arange(1, 5, dtype=np.complex64).reshape(2, 2) * (1 + 1j)
    layer = expect_grid_to_layer(g, 4)
    assert layer[0, 0] == g[1, 1] and layer[3, 3] == g[0, 0] and layer[0, 3] == g[1, 0] and layer[3, 0] == g[0, 1]
    assert np.count_nonzero(layer) == 4
    np.testing.assert_array_equal(expect_layer_to_grid(layer, 2), g)
    # the Hermitian half: its real inverse transform is the real part of the layer's
    g = (rs.standard_normal((6, 6)) + 1j * rs.standard_normal((6, 6))).astype(np.complex64)
    half = expect_half_layer(g, 8)
    np.testing.assert_allclose(np.fft.irfft2(half, s=(8, 8)), np.fft.ifft2(expect_grid_to_layer(g, 8)).real,
                               atol=1e-6)
    spectrum = np.fft.rfft2(rs.standard_normal((8, 8))).astype(np.complex64)
    full = np.fft.fft2(np.fft.irfft2(spectrum.astype(np.complex128), s=(8, 8)))
    np.testing.assert_allclose(expect_half_layer_to_grid(spectrum, 6), expect_layer_to_grid(full, 6), atol=1e-5)
    # layer <-> image against the oracle's whole routes (float64, w != 0)
    G, w = 8, 3.0
    k = rs.uniform(0.5, 2.0, G)
    scale, bias = 0.05, -0.2
    grid = rs.standard_normal((1, G, G)) + 1j * rs.standard_normal((1, G, G))
    image = np.zeros((1, G, G))
    layer = np.fft.ifft2(np.fft.ifftshift(grid[0])) * G * G
    orc.grid_to_image(grid.copy(), image, k, scale, bias, w)
    want, bound = expect_layer_to_image(np.zeros((G, G)), layer, k, scale, bias, w)
    np.testing.assert_allclose(want.astype(np.float64), image[0], rtol=1e-9, atol=1e-9)
    assert bound.max() < 1e-12
    back, _ = orc.image_to_grid(image, k, scale, bias, w, np.complex128)
    layer, bound = expect_image_to_layer(image[0], k, scale, bias, w)
    np.testing.assert_allclose(expect_layer_to_grid(np.fft.fft2(layer.astype(np.complex128)), G), back[0],
                               rtol=1e-9, atol=1e-9)
    want, _ = expect_fourier_beam(np.ones((4, 3), np.complex64), 2.0, -0.5, 0.25, -1.0)
    assert abs(want[3, 2] - 2.0 * math.exp((-0.5 * -1 + 0.25 * 2) * -1 - 4.0)) < 1e-12
    uv, wts, N = weights_stream(6, 10, 2, 1)
    got = expect_grid_weights(np.zeros((2, 6, 10), np.float32), uv, wts, N)
    assert got.sum() == wts[:N].sum() and got[:, 5, 9].min() >= wts[N - 5:N].sum(axis=0).min()
    assert got[0, 0, 0] > 0 and got[0, 0, 9] > 0 and got[0, 5, 0] > 0
    # the route truths: the oracle's routes agree with the module whose bound they are held to
    G, Gg, w = 16, 6, 3.0
    k = rs.uniform(0.5, 2.0, G).astype(np.float32)
    scale = np.float32(0.9 / G)
    bias = np.float32(-0.5 * G * float(scale))
    g = cplx(rs, (Gg, Gg), np.complex64)
    truth, allowed, corr = expect_grid_to_image('g2i_w', g, G, k, scale, bias, w)
    other, _ = tt.transform_truth64('g2i_w', G, Gg, grid=g, kernel1d=k, lm_scale=scale, lm_bias=bias, w=w)
    assert np.linalg.norm((truth - other) / corr) < 0.1 * allowed
    m = rs.standard_normal((G, G)).astype(np.float32)
    truth, allowed = expect_image_to_grid('i2g_w', m, Gg, k, scale, bias, w)
    other, _ = tt.transform_truth64('i2g_w', G, Gg, image=m, kernel1d=k, lm_scale=scale, lm_bias=bias, w=w)
    assert np.linalg.norm(truth - other) < 0.1 * allowed
    truth, coeff, allowed = expect_convolve_beam(m)
    other, _ = tt.transform_truth64('beam', G, image=m, beam=coeff)
    assert np.linalg.norm(truth - other) < 0.1 * allowed
    # the refusals' positive control: the same calls with the stride set to the width pass the
    # argument checks, so the stride is what the GPU test's KIMG_EINVAL is about.  Only without a
    # device, where the first HIP call then fails: with one, these dummy pointers would be used.
    import torch
    if not torch.cuda.is_available():
        class Fake:
            ptr, row, pol = 1 << 20, 68, 67 * 68
        for name, fn in _refusals(64).items():
            assert fn(Fake, Fake) != KIMG_EINVAL, name
        for name, fn in _refusals(63).items():
            assert fn(Fake, Fake) == KIMG_EINVAL, name
    # every strided entry point is refused somewhere below, except the two that take no width
    assert strided_entry_points_without_refusal() == {'kimg_find_peak', 'kimg_find_peak_masked'}


# ---------------------------------------------------------------------------------------------
# GPU harness

def L():
    from katsdpimager_amd._lib import lib
    return lib()


def ok(rc):
    assert rc == 0, rc


def dev(a):
    from katsdpimager_amd import accel
    ctx, q = context_queue()
    a = np.ascontiguousarray(a)
    d = accel.DeviceArray(ctx, a.shape, a.dtype)
    d.set(q, a)
    return d


def padded(inner, layout, which=0, **kw):
    ctx, q = context_queue()
    return Padded(ctx, q, inner, **dict(LAYOUTS[layout][which], **kw))


def strides(p):
    return p.ptr, p.row, p.pol


def image_args(p):
    P, H, W = p.shape
    return p.ptr, p.row, p.pol, W, H, P


def guarded(values, front, dtype=None):
    """A 1-D array as a [1][1][n] Padded with `front` sentinel elements before it and 5 behind."""
    ctx, q = context_queue()
    values = np.asarray(values, dtype)
    return Padded(ctx, q, values.reshape(1, 1, -1), rpad=5, vpad=1, origin=(0, front))


def image_of(H, W, P, seed, dtype=np.float32):
    return np.random.RandomState(seed).standard_normal((P, H, W)).astype(dtype)


# ---------------------------------------------------------------------------------------------
# elementwise operators: numpy in the same dtype, exact

@gpu
@layouts
@shapes
def test_scale(H, W, P, layout):
    ctx, q = context_queue()
    src = image_of(H, W, P, 1)
    sf = np.array([1.2, 2.3, 3.4, -4.5], np.float32)[:P]
    p = padded(src, layout)
    ok(L().kimg_scale(*image_args(p), (ctypes.c_float * P)(*sf), q.handle))
    np.testing.assert_array_equal(p.get(q), src * sf[:, None, None])
    # factors on the device, made there from a pixel of the last row and column
    p = padded(src, layout)
    out = guarded(np.zeros(P, np.float32), 3)
    ok(L().kimg_pixel_reciprocal(*image_args(p), W - 1, H - 1, out.ptr, q.handle))
    ok(L().kimg_scale_device(*image_args(p), out.ptr, q.handle))
    recip = np.float32(1) / src[:, H - 1, W - 1]
    np.testing.assert_array_equal(out.get(q)[0, 0], recip)
    np.testing.assert_array_equal(p.get(q), src * recip[:, None, None])
    src64 = image_of(H, W, P, 2, np.float64)
    sf64 = np.array([1.2, 2.3, 3.4, -4.5])[:P]
    p = padded(src64, layout)
    ok(L().kimg_scale_f64(*image_args(p), (ctypes.c_double * P)(*sf64), q.handle))
    np.testing.assert_array_equal(p.get(q), src64 * sf64[:, None, None])


@gpu
@layouts
@shapes
def test_add_image(H, W, P, layout):
    ctx, q = context_queue()
    for dtype, fn in ((np.float32, L().kimg_add_image), (np.float64, L().kimg_add_image_f64)):
        dest, src = image_of(H, W, P, 3, dtype), image_of(H, W, P, 4, dtype)
        d, s = padded(dest, layout, 0), padded(src, layout, 1)
        ok(fn(*strides(d), *strides(s), W, H, P, q.handle))
        np.testing.assert_array_equal(d.get(q), dest + src)
        np.testing.assert_array_equal(s.get(q), src)


@gpu
@layouts
@shapes
def test_apply_primary_beam(H, W, P, layout):
    """Beam values below, at and above the threshold; the beam's row stride differs from the
    image's."""
    ctx, q = context_queue()
    for dtype, fn in ((np.float32, L().kimg_apply_primary_beam), (np.float64, L().kimg_apply_primary_beam_f64)):
        rs = np.random.RandomState(5)
        src = image_of(H, W, P, 6, dtype)
        beam = rs.uniform(0.0, 1.0, (H, W)).astype(dtype)
        threshold = dtype(0.2)
        beam[0, 0] = beam[H - 1, W - 1] = beam[H // 2, W - 1] = threshold                   # at
        beam[0, 1] = np.nextafter(threshold, dtype(0))                                      # just below
        beam[H - 1, 0] = np.nextafter(threshold, dtype(1))                                  # just above
        assert (beam < threshold).sum() > 3 and (beam > threshold).sum() > 3
        d, b = padded(src, layout, 0), padded(beam, layout, 1)
        assert d.row != b.row
        ok(fn(*strides(d), b.ptr, b.row, W, H, P, float(threshold), 12345.0, q.handle))
        np.testing.assert_array_equal(d.get(q), expect_primary_beam(src, beam, threshold, 12345.0))
        np.testing.assert_array_equal(b.get(q), beam)


@gpu
@pytest.mark.parametrize('count', [1, 3, 4, 5, 1027, 5000000])
def test_fill(count):
    """Every count & 3 tail; 5000000 takes the grid-stride loop's second round (more than 2048
    blocks of 1024 elements).  The data pointer keeps the 16-byte alignment kimg_fill asks for
    (include/kimg.h; weight.hip refuses anything else): 4 sentinel floats in front."""
    ctx, q = context_queue()
    assert -(-count // 1024) > 2048 or count < 2048 * 1024
    p = guarded(np.full(count, 7.0, np.float32), 4)
    assert p.ptr % 16 == 0
    ok(L().kimg_fill(p.ptr, count, -2.5, q.handle))
    got = p.get(q)
    assert got.shape == (1, 1, count) and np.all(got == np.float32(-2.5))
    assert L().kimg_fill(p.ptr + 4, count, 1.0, q.handle) == KIMG_EINVAL
    assert np.all(p.get(q) == np.float32(-2.5))


@gpu
@pytest.mark.parametrize('count', [1, 3, 1027])
def test_real_to_complex(count):
    """dst[i] = (src[i], 0) between sentinels, both pointers only element-aligned."""
    ctx, q = context_queue()
    src = np.random.RandomState(count).standard_normal(count).astype(np.float32)
    s = guarded(src, 1)
    d = guarded(np.full(count, 9 + 9j, np.complex64), 1)
    ok(L().kimg_real_to_complex(d.ptr, s.ptr, count, q.handle))
    np.testing.assert_array_equal(d.get(q)[0, 0], src.astype(np.complex64))
    np.testing.assert_array_equal(s.get(q)[0, 0], src)


@gpu
@layouts
@pytest.mark.parametrize('H,W', [(300, 302), (6, 10)])
def test_fourier_beam(H, W, layout):
    """complex64 [H][W] half spectrum with a padded row stride, in place."""
    ctx, q = context_queue()
    rs = np.random.RandomState(7)
    data = (rs.standard_normal((H, W)) + 1j * rs.standard_normal((H, W))).astype(np.complex64)
    coeff = (1.5, -2e-4, 1e-4, -3e-4)
    p = padded(data, layout)
    ok(L().kimg_fourier_beam(p.ptr, p.row, W, H, *coeff, q.handle))
    want, bound = expect_fourier_beam(data, *coeff)
    got = p.get(q).astype(np.complex128)
    assert np.all(np.abs(got.real - want.real) <= bound) and np.all(np.abs(got.imag - want.imag) <= bound)


# ---------------------------------------------------------------------------------------------
# statistics

@gpu
@layouts
@shapes
def test_image_peak(H, W, P, layout):
    """orc.find_peak, exact.  The largest admissible value (15 + 1 ulp where pbeam = 0.5: the
    product just clears 7.5 * noise) sits in the last column, negative; a larger one (20 where
    pbeam = 0.375: exactly 7.5, not above) in the last row of the last polarization: with the beam
    the first is the peak, without it the second.  NaNs in image and beam never pass."""
    ctx, q = context_queue()
    rs = np.random.RandomState(8)
    noise = 1.0
    image = (0.3 * rs.standard_normal((P, H, W))).astype(np.float32)
    pbeam = rs.uniform(0.3, 1.0, (H, W)).astype(np.float32)
    a = (0, 2, W - 1)
    b = (P - 1, H - 1, 3)
    image[a] = -np.nextafter(np.float32(15), np.float32(16))
    pbeam[a[1:]] = 0.5
    image[b] = 20.0
    pbeam[b[1:]] = 0.375
    image[0, 1, 1] = np.nan
    image[P - 1, 3, 2] = 100.0
    pbeam[3, 2] = np.nan
    assert image[b] * pbeam[b[1:]] == np.float32(7.5 * noise) and abs(image[a]) * pbeam[a[1:]] > 7.5 * noise
    img, beam = padded(image, layout, 0), padded(pbeam, layout, 1)
    peak = guarded(np.full(1, 55.0, np.float32), 1)
    ok(L().kimg_image_peak(*strides(img), beam.ptr, beam.row, W, H, P, noise, peak.ptr, q.handle))
    want = orc.find_peak(image, pbeam, noise)
    assert want == abs(image[a])
    assert peak.get(q)[0, 0, 0] == want
    # no pixel qualifies: 0 (the reference's NaN)
    ok(L().kimg_image_peak(*strides(img), beam.ptr, beam.row, W, H, P, 50.0, peak.ptr, q.handle))
    assert np.isnan(orc.find_peak(image, pbeam, 50.0)) and peak.get(q)[0, 0, 0] == 0.0
    # without a beam
    ok(L().kimg_image_peak(*strides(img), None, 0, W, H, P, noise, peak.ptr, q.handle))
    want = orc.find_peak(image, np.ones((H, W), np.float32), noise)
    assert want == 100.0 and peak.get(q)[0, 0, 0] == want
    image[P - 1, 3, 2] = 1.0
    img = padded(image, layout, 0)
    ok(L().kimg_image_peak(*strides(img), None, 0, W, H, P, noise, peak.ptr, q.handle))
    assert peak.get(q)[0, 0, 0] == 20.0 == orc.find_peak(image, np.ones((H, W), np.float32), noise)
    img.get(q)
    beam.get(q)


@gpu
@layouts
@shapes
def test_image_nansum(H, W, P, layout):
    """math.fsum of the non-NaN interior per polarization, within n 2^-52 fsum(|x|); NaNs skipped;
    an infinity (+ in one polarization, - in the next) decides its sum."""
    ctx, q = context_queue()
    rs = np.random.RandomState(9)
    image = (rs.standard_normal((P, H, W)) * 10.0 ** rs.randint(-3, 4, (P, H, W))).astype(np.float32)
    image[rs.uniform(size=image.shape) < 0.05] = np.nan
    image[:, H - 1, W - 1] = 1e6
    image[:, 0, W - 1] = -3e5
    for with_inf in (False, True):
        if with_inf:
            image[0, H // 2, W - 1] = np.inf
            if P > 1:
                image[1, H - 1, W // 2] = -np.inf
        img = padded(image, layout)
        sums = guarded(np.full(P, 5.0), 1)
        ok(L().kimg_image_nansum(*image_args(img), sums.ptr, q.handle))
        got = sums.get(q)[0, 0]
        want, bound = expect_nansum(image)
        for p in range(P):
            if np.isinf(want[p]):
                assert got[p] == want[p]
            else:
                assert abs(got[p] - want[p]) <= bound[p], (p, got[p], want[p], bound[p])
        img.get(q)


@gpu
@layouts
@pytest.mark.parametrize('H,W,P', [(300, 302, 1), (300, 302, 4), (6, 10, 3), (6, 10, 2)])
def test_psf_patch(H, W, P, layout):
    """orc.psf_patch, exact, with and without a limit, on a non-square PSF; the pixels that
    decide the box sit in different polarizations."""
    ctx, q = context_queue()
    rs = np.random.RandomState(10)
    psf = (0.01 * rs.uniform(-1, 1, (P, H, W))).astype(np.float32)
    my, mx = H // 2, W // 2
    psf[:, my, mx] = 1.0
    psf[0, my - min(40, my), mx + 1] = -0.5
    psf[P - 1, my + 1, mx + min(57, mx - 1)] = 0.3
    psf[0, 0, 0] = 0.9                  # (outside the limit's region)
    p = padded(psf, layout)
    for threshold, limit in ((0.25, None), (0.25, 0.5), (0.05, 0.9), (5.0, None)):
        min_x, min_y, max_x, max_y = 0, 0, W - 1, H - 1
        if limit is not None:
            hl = (round(limit * min(H, W)) - 1) // 2
            min_x, min_y, max_x, max_y = max(0, mx - hl), max(0, my - hl), min(W - 1, mx + hl), min(H - 1, my + hl)
        bound = guarded(np.full(2, 77, np.int32), 1, np.int32)
        ok(L().kimg_psf_patch(p.ptr, p.row, p.pol, P, min_x, min_y, max_x, max_y, mx, my, threshold,
                              bound.ptr, q.handle))
        b = bound.get(q)[0, 0]
        box = (P, int(min(2 * b[1] + 1, H)), int(min(2 * b[0] + 1, W)))
        want = orc.psf_patch(psf, threshold, limit)
        if limit is not None:
            # (the oracle clamps to the limited region's size, the wrapper to the image's)
            want = (want[0], min(want[1], H), min(want[2], W))
            box = (box[0], min(box[1], max_y - min_y + 1), min(box[2], max_x - min_x + 1))
        assert box == want, (threshold, limit, b, want)
    p.get(q)


def noise_case(case, H, W, P, border, rs):
    img = rs.standard_normal((P, H, W)).astype(np.float32)
    if case == 1:
        img = (np.round(img * 3) / 3).astype(np.float32)       # many exact ties around the median
    elif case == 4:
        # the two middle elements part at the first byte: half of the interior is zero
        inner = img[:, border:H - border, border:W - border]
        flat = np.abs(inner).ravel() + np.float32(1e3)
        flat[rs.permutation(flat.size)[:flat.size // 2]] = 0.0
        inner[...] = flat.reshape(inner.shape)
    return img


@gpu
@layouts
@pytest.mark.parametrize('case', [1, 4])
@pytest.mark.parametrize('H,W,P,border', [(300, 302, 1, 7), (300, 302, 4, 30), (6, 10, 3, 1)])
def test_noise_selection(H, W, P, border, case, layout):
    """kimg_noise_est is np.median(|x| inside the border) * 1.4826 in float32, exactly (cases 1
    and 4 of test_noise_est_device_selection: ties; the middle elements part at the first byte);
    kimg_abs_histogram and kimg_abs_count_le are numpy's counts of the same region, exactly.  The
    border region holds huge values too."""
    ctx, q = context_queue()
    rs = np.random.RandomState(H + P + case)
    image = noise_case(case, H, W, P, border, rs)
    frame = np.ones((H, W), bool)
    frame[border:H - border, border:W - border] = False
    image[:, frame] = 1e30
    img = padded(image, layout)
    scratch = dev(np.zeros(L().kimg_noise_est_scratch_bytes() // 4 + 1, np.uint32))
    out = guarded(np.zeros(1, np.float32), 1)
    ok(L().kimg_noise_est(*image_args(img), border, float(np.float32(orc.MEDIAN_TO_RMS)), scratch.ptr,
                          out.ptr, q.handle))
    assert out.get(q)[0, 0, 0] == expect_noise(image, border)
    inner = np.abs(image[:, border:H - border, border:W - border])
    median_bits = int(np.sort(inner.ravel())[(inner.size - 1) // 2].view(np.uint32))
    hist = guarded(np.full(256, 9, np.uint32), 1, np.uint32)
    for pass_ in (3, 2, 0):
        prefix = median_bits >> (8 * (pass_ + 1))
        ok(L().kimg_abs_histogram(*image_args(img), border, pass_, prefix, hist.ptr, q.handle))
        want = expect_histogram(image, border, pass_, prefix)
        assert want.sum() > 0
        np.testing.assert_array_equal(hist.get(q)[0, 0], want)
    count = guarded(np.full(2, 9, np.uint32), 1, np.uint32)
    for value in (np.uint32(median_bits).view(np.float32), np.float32(0.0), np.float32(1e31)):
        ok(L().kimg_abs_count_le(*image_args(img), border, float(value), count.ptr, q.handle))
        np.testing.assert_array_equal(count.get(q)[0, 0], expect_count_le(image, border, value))
    img.get(q)


# ---------------------------------------------------------------------------------------------
# weights

@gpu
@layouts
@pytest.mark.parametrize('H,W,P', [(300, 302, 1), (300, 302, 2), (300, 302, 3), (300, 302, 4), (6, 10, 3)])
def test_grid_weights(H, W, P, layout):
    """orc.weights_grid_add on a prefilled grid, exactly (integer weights)."""
    ctx, q = context_queue()
    uv, weights, N = weights_stream(H, W, P, 11)
    prefill = np.random.RandomState(12).randint(0, 4, (P, H, W)).astype(np.float32)
    g = padded(prefill, layout)
    d_uv, d_weights = dev(uv), dev(weights)        # (held until the call has run)
    ok(L().kimg_grid_weights(*image_args(g), d_uv.ptr, d_weights.ptr, N, q.handle))
    want = expect_grid_weights(prefill, uv, weights, N)
    assert want.max() < 2 ** 24
    np.testing.assert_array_equal(g.get(q), want)


@gpu
@layouts
@pytest.mark.parametrize('H,W,P', [(300, 302, 1), (300, 302, 4), (6, 10, 3), (500, 2100, 2)])
def test_density_weights(H, W, P, layout):
    """kimg_mean_weight's two sums and kimg_density_weights' three against math.fsum within
    n 2^-52 fsum(|x|); the density grid against orc.weights_finalize (robust) at rtol 2e-5; the
    one-call robust form against the two steps with `a` made on the host as include/kimg.h says.
    Cells without visibilities stay exactly 0."""
    ctx, q = context_queue()
    rs = np.random.RandomState(13)
    weights = rs.uniform(0.1, 2.0, (P, H, W)).astype(np.float32)
    weights[rs.uniform(size=weights.shape) < 0.4] = 0.0
    weights[:, H - 1, W - 1] = 1.5
    robustness = 0.5
    robust = (5 * 10 ** (-robustness)) ** 2
    g = padded(weights, layout)
    mean_sums = guarded(np.full(2, 3.0), 2)
    ok(L().kimg_mean_weight(mean_sums.ptr, g.ptr, g.row, W, H, q.handle))
    ms = mean_sums.get(q)[0, 0]
    w0 = weights[0].astype(np.float64).ravel()
    for got, terms in zip(ms, (w0, w0 * w0)):
        assert abs(got - math.fsum(terms)) <= fsum_bound(terms), (got, math.fsum(terms))
    np.testing.assert_array_equal(g.get(q), weights)
    a = float(np.float32(robust / (ms[1] / ms[0])))
    want_d, want_sums, bounds = expect_density(weights, a, 1.0)
    ref = weights.copy()
    orc.weights_finalize(orc.ROBUST, ref, robustness)
    results = []
    for form in ('two_step', 'robust'):
        g = padded(weights, layout)
        sums = guarded(np.full(3, 3.0), 2)
        if form == 'two_step':
            ok(L().kimg_density_weights(sums.ptr, *image_args(g), a, 1.0, q.handle))
        else:
            ok(L().kimg_density_weights_robust(sums.ptr, *image_args(g), mean_sums.ptr, robust, 1.0, q.handle))
        got = g.get(q)
        np.testing.assert_allclose(got, ref, rtol=2e-5, atol=0)
        assert np.all(got[weights == 0] == 0)
        s = sums.get(q)[0, 0]
        assert np.all(np.abs(s - want_sums) <= bounds), (form, s, want_sums, bounds)
        results.append(got)
    np.testing.assert_array_equal(results[0], results[1])
    np.testing.assert_array_equal(results[0], want_d)


# ---------------------------------------------------------------------------------------------
# grid <-> layer <-> image pieces (square by contract)

SIZES = [(16, 6), (64, 64), (120, 50), (126, 126)]
sizes = pytest.mark.parametrize('G,Gg', SIZES)


def cplx(rs, shape, dtype):
    return (rs.standard_normal(shape) + 1j * rs.standard_normal(shape)).astype(dtype)


@gpu
@layouts
@sizes
def test_layer_copies(G, Gg, layout):
    """numpy slicing, exact: the zero-padded corner-DC layer of a padded grid and back, complex64
    and complex128.  The layer is dense by contract; its buffer starts full of sentinels (the
    call zeroes what the grid does not reach)."""
    ctx, q = context_queue()
    for dtype, to_layer, to_grid in ((np.complex64, L().kimg_grid_to_layer, L().kimg_layer_to_grid),
                                     (np.complex128, L().kimg_grid_to_layer_f64, L().kimg_layer_to_grid_f64)):
        rs = np.random.RandomState(G)
        grid = cplx(rs, (Gg, Gg), dtype)
        g = padded(grid, layout)
        # (dense rows: only whole sentinel rows in front and behind)
        layer = padded(np.full((G, G), 5 - 5j, dtype), layout, rpad=0, vpad=1, origin=(1, 0))
        assert layer.row == G
        ok(to_layer(layer.ptr, G, g.ptr, g.row, Gg, q.handle))
        np.testing.assert_array_equal(layer.get(q), expect_grid_to_layer(grid, G))
        np.testing.assert_array_equal(g.get(q), grid)
        full = cplx(rs, (G, G), dtype)
        src = dev(full)
        out = padded(np.full((Gg, Gg), 5 - 5j, dtype), layout)
        ok(to_grid(out.ptr, out.row, Gg, src.ptr, G, q.handle))
        np.testing.assert_array_equal(out.get(q), expect_layer_to_grid(full, Gg))


@gpu
@layouts
@sizes
def test_half_layer_copies(G, Gg, layout):
    """The Hermitian half layer of a padded grid (fl(0.5 (g(k) + conj g(-k))) per component) and
    the grid from a half spectrum (F(-k) = conj F(k)), exact against numpy."""
    ctx, q = context_queue()
    rs = np.random.RandomState(G + 1)
    grid = cplx(rs, (Gg, Gg), np.complex64)
    g = padded(grid, layout)
    half = padded(np.full((G, G // 2 + 1), 5 - 5j, np.complex64), layout, rpad=0, vpad=1, origin=(1, 0))
    ok(L().kimg_grid_to_half_layer(half.ptr, G, g.ptr, g.row, Gg, q.handle))
    np.testing.assert_array_equal(half.get(q), expect_half_layer(grid, G))
    g.get(q)
    spectrum = cplx(rs, (G, G // 2 + 1), np.complex64)
    out = padded(np.full((Gg, Gg), 5 - 5j, np.complex64), layout)
    d_spectrum = dev(spectrum)
    ok(L().kimg_half_layer_to_grid(out.ptr, out.row, Gg, d_spectrum.ptr, G, q.handle))
    np.testing.assert_array_equal(out.get(q), expect_half_layer_to_grid(spectrum, Gg))


@gpu
@layouts
@pytest.mark.parametrize('w', [0.0, 3.0, -12.25])
@pytest.mark.parametrize('G', [16, 64, 120, 126])
def test_layer_image(G, w, layout):
    """kimg_layer_to_image accumulates into a prefilled, padded image; kimg_image_to_layer reads
    one.  float32 and float64, against the float64 evaluation of expect_layer_to_image /
    expect_image_to_layer within the bounds derived there."""
    ctx, q = context_queue()
    for real, cdt, to_image, to_layer in (
            (np.float32, np.complex64, L().kimg_layer_to_image, L().kimg_image_to_layer),
            (np.float64, np.complex128, L().kimg_layer_to_image_f64, L().kimg_image_to_layer_f64)):
        rs = np.random.RandomState(G)
        k1d = rs.uniform(0.5, 2.0, G).astype(real)
        lm_scale = real(0.9 / G)
        lm_bias = real(-0.5 * G * float(lm_scale))
        layer = cplx(rs, (G, G), cdt)
        prefill = rs.standard_normal((G, G)).astype(real)
        img = padded(prefill, layout)
        d_layer, d_k1d = dev(layer), dev(k1d)
        ok(to_image(img.ptr, img.row, d_layer.ptr, G, d_k1d.ptr, float(lm_scale), float(lm_bias), w, q.handle))
        want, bound = expect_layer_to_image(prefill, layer, k1d, lm_scale, lm_bias, w)
        got = img.get(q).astype(WIDE)
        assert np.all(np.abs(got - want) <= bound)
        out = padded(np.full((G, G), 5 - 5j, cdt), layout, rpad=0, vpad=1, origin=(1, 0))
        img = padded(prefill, layout)
        ok(to_layer(out.ptr, img.ptr, img.row, G, d_k1d.ptr, float(lm_scale), float(lm_bias), w, q.handle))
        want, bound = expect_image_to_layer(prefill, k1d, lm_scale, lm_bias, w)
        got = out.get(q).astype(np.clongdouble)
        assert np.all(np.abs(got.real - want.real) <= bound) and np.all(np.abs(got.imag - want.imag) <= bound)
        img.get(q)


@gpu
@layouts
@pytest.mark.parametrize('G', [16, 64, 120, 126])
def test_real_layer_image(G, layout):
    """The w = 0 pair on real layers with rows of G + 2 floats (and a padded image): every step is
    a correctly rounded float32 operation without contraction, so numpy's float32 gives the same
    bits."""
    ctx, q = context_queue()
    rs = np.random.RandomState(G + 2)
    k1d = rs.uniform(0.5, 2.0, G).astype(np.float32)
    lm_scale = np.float32(0.9 / G)
    lm_bias = np.float32(-0.5 * G * float(lm_scale))
    n, t, _ = correction(G, k1d, lm_scale, lm_bias, 0.0, np.float32)
    layer = rs.standard_normal((G, G)).astype(np.float32)
    prefill = rs.standard_normal((G, G)).astype(np.float32)
    img = padded(prefill, layout)
    lay = padded(layer, layout, 1, rpad=2 + LAYOUTS[layout][1]['rpad'])
    d_k1d = dev(k1d)
    ok(L().kimg_real_layer_to_image(img.ptr, img.row, lay.ptr, lay.row, G, d_k1d.ptr, float(lm_scale),
                                    float(lm_bias), q.handle))
    np.testing.assert_array_equal(img.get(q), prefill + (np.fft.fftshift(layer) * n) / t)
    lay.get(q)
    img = padded(prefill, layout)
    lay = padded(np.full((G, G), 5.0, np.float32), layout, 1)
    ok(L().kimg_image_to_real_layer(lay.ptr, lay.row, img.ptr, img.row, G, d_k1d.ptr, float(lm_scale),
                                    float(lm_bias), q.handle))
    np.testing.assert_array_equal(lay.get(q), np.fft.ifftshift(prefill / (t * n)))
    img.get(q)


# ---------------------------------------------------------------------------------------------
# the whole routes on the library's own transforms

ROUTE_SIZES = [(G, Gg) for G, Gg in SIZES if tt.supported(G, Gg)]


def workspace(op, G, Gg):
    """(dense device array, bytes): the workspace keeps the 16-byte alignment include/kimg.h asks
    of it (the allocator's; asserted)."""
    nbytes = tt.workspace_bytes(op, G, Gg)
    ws = dev(np.zeros(nbytes // 4 + 4, np.float32))
    assert ws.ptr % 16 == 0
    return ws, nbytes


@gpu
@layouts
@pytest.mark.parametrize('w', [0.0, 3.0, -12.25])
@pytest.mark.parametrize('G,Gg', ROUTE_SIZES)
def test_routes(G, Gg, w, layout):
    """kimg_grid_to_image_real / _w and kimg_image_to_grid_real / _w with differently padded grid
    and image (each with origin (1, 1) in one layout) against helpers.grid_to_image_truth and the
    float64 orc.image_to_grid, held to the norm-wise bound tests/test_transform_truth.py asserts
    for the route at that size (transform_bound).  Grid -> image overwrites (accumulate 0, onto
    a prefill) and accumulates; image -> grid overwrites every cell of a prefilled grid and, the
    padding check says, nothing beyond grid_size in a row.  The w = 0 routes run at w = 0 only."""
    ctx, q = context_queue()
    assert ROUTE_SIZES == SIZES
    rs = np.random.RandomState(G + Gg)
    k1d = rs.uniform(0.5, 2.0, G).astype(np.float32)
    lm_scale = np.float32(0.9 / G)
    lm_bias = np.float32(-0.5 * G * float(lm_scale))
    d_k1d = dev(k1d)
    grid = cplx(rs, (Gg, Gg), np.complex64)
    prefill = rs.standard_normal((G, G)).astype(np.float32)
    image = rs.uniform(-1, 1, (G, G)).astype(np.float32)
    coords = (float(lm_scale), float(lm_bias))
    for op in (('g2i_real', 'g2i_w') if w == 0 else ('g2i_w',)):
        ws, nbytes = workspace(op, G, Gg)
        for accumulate in (0, 1):
            img, g = padded(prefill, layout, 0), padded(grid, layout, 1)
            if op == 'g2i_real':
                ok(L().kimg_grid_to_image_real(img.ptr, img.row, G, g.ptr, g.row, Gg, d_k1d.ptr, *coords,
                                               accumulate, ws.ptr, nbytes, q.handle))
            else:
                ok(L().kimg_grid_to_image_w(img.ptr, img.row, G, g.ptr, g.row, Gg, d_k1d.ptr, *coords, w,
                                            accumulate, ws.ptr, nbytes, q.handle))
            truth, allowed, corr = expect_grid_to_image(op, grid, G, k1d, lm_scale, lm_bias, w,
                                                        prefill if accumulate else None)
            got = img.get(q).astype(np.float64)
            assert np.linalg.norm((got - truth) / corr) < allowed, (op, accumulate)
            np.testing.assert_array_equal(g.get(q), grid)
    for op in (('i2g_real', 'i2g_w') if w == 0 else ('i2g_w',)):
        ws, nbytes = workspace(op, G, Gg)
        img, g = padded(image, layout, 0), padded(np.full((Gg, Gg), 9 - 4j, np.complex64), layout, 1)
        if op == 'i2g_real':
            ok(L().kimg_image_to_grid_real(g.ptr, g.row, Gg, img.ptr, img.row, G, d_k1d.ptr, *coords,
                                           ws.ptr, nbytes, q.handle))
        else:
            ok(L().kimg_image_to_grid_w(g.ptr, g.row, Gg, img.ptr, img.row, G, d_k1d.ptr, *coords, w,
                                        ws.ptr, nbytes, q.handle))
        truth, allowed = expect_image_to_grid(op, image, Gg, k1d, lm_scale, lm_bias, w)
        got = g.get(q).astype(np.complex128)
        assert np.linalg.norm(got - truth) < allowed, op
        np.testing.assert_array_equal(img.get(q), image)


@gpu
@layouts
@pytest.mark.parametrize('G', [16, 64, 120, 126])
def test_convolve_beam(G, layout):
    """kimg_convolve_beam in place on a padded image against the float64 orc.convolve_beam, within
    the norm-wise bound of tests/test_transform_truth.py for the beam at that size."""
    ctx, q = context_queue()
    rs = np.random.RandomState(G)
    model = np.zeros((G, G), np.float32)
    for _ in range(50):
        model[rs.randint(G), rs.randint(G)] += rs.uniform(-1, 2)
    model += (0.01 * rs.standard_normal((G, G))).astype(np.float32)
    truth, coeff, allowed = expect_convolve_beam(model)
    ws, nbytes = workspace('beam', G, G)
    img = padded(model, layout)
    ok(L().kimg_convolve_beam(img.ptr, img.row, G, *coeff, ws.ptr, nbytes, q.handle))
    assert np.linalg.norm(img.get(q).astype(np.float64) - truth) < allowed


# ---------------------------------------------------------------------------------------------
# gridder and degridder on sub-image pointers (the integer cases of tests/test_exact_gridding.py:
# every variant and form equals the float64 truth bit for bit)

def _case(cases, name):
    return next(c for c in cases if c.name == name)


def gridder_workspace(fn, *args):
    nbytes = int(fn(*args))
    ws = dev(np.zeros(max(nbytes, 16), np.uint8))
    return ws, nbytes


@gpu
@layouts
@pytest.mark.parametrize('precision', ['f32', 'f64'])
@pytest.mark.parametrize('name', ['k7_edges', 'k16_ov16_p4_moves'])
def test_gridders(name, precision, layout):
    """kimg_grid (generic, window kernel in its three arithmetic forms, binned) and kimg_grid_f64
    (generic, window, binned) add to a prefilled, padded grid whose interior, or whose density
    weights' interior, starts at row 1, column 1 of its buffer: prefill + truth, exactly."""
    from katsdpimager_amd import grid as kgrid
    ctx, q = context_queue()
    case = _case(eg.GRID_CASES, name)
    inp, want, bound = eg._grid_case(case)
    P, G, K, W, OV = case.P, case.G, case.K, case.W, case.OV
    n = len(inp['uv'])
    prefill = eg._cint(np.random.RandomState(5), want.shape, 100)
    assert bound.max() + 200 < eg.EXACT
    table, uv, wp, vis = dev(inp['kern']), dev(inp['uv']), dev(inp['w_plane']), dev(inp['vis'])
    if precision == 'f32':
        runs = [('generic', 'fp32'), ('binned', 'fp32')] + [('mfma', a) for a in eg.GRID_FORMS]
    else:
        runs = [('generic', None), ('mfma', None), ('binned', None)]
    for variant, arith in runs:
        cdt = np.complex64 if precision == 'f32' else np.complex128
        g, wg = padded(prefill.astype(cdt), layout, 0), padded(inp['wg'], layout, 1)
        size = L().kimg_grid_binned_workspace_bytes if variant == 'binned' else L().kimg_grid_workspace_bytes
        ws, nbytes = gridder_workspace(size, n, P, W, OV, K)
        head = (g.ptr, g.row, g.pol, G, P, wg.ptr, wg.row, wg.pol, uv.ptr, wp.ptr, vis.ptr, n, table.ptr, W, OV, K,
                ws.ptr, nbytes, kgrid.GRID_VARIANTS[variant])
        if precision == 'f32':
            ok(L().kimg_grid(*head, kgrid.GRID_ARITH[arith], q.handle))
        else:
            ok(L().kimg_grid_f64(*head, q.handle))
        eg._assert_exact(g.get(q), want + prefill, '%s/%s' % (variant, arith))
        np.testing.assert_array_equal(wg.get(q), inp['wg'])


@gpu
@layouts
@pytest.mark.parametrize('precision', ['f32', 'f64'])
@pytest.mark.parametrize('name', ['dk7_edges', 'dk16_ov16_p4_moves'])
def test_degridders(name, precision, layout):
    """kimg_degrid (generic, window kernel in both forms, binned) and kimg_degrid_f64 read a padded
    grid through a sub-image pointer: the float64 truth, exactly."""
    from katsdpimager_amd import grid as kgrid
    ctx, q = context_queue()
    case = _case(eg.DEGRID_CASES, name)
    inp, want, bound = eg._degrid_case(case)
    P, G, K, W, OV = case.P, case.G, case.K, case.W, case.OV
    n = len(inp['uv'])
    assert bound.max() < eg.EXACT
    table, uv, wp, weights = dev(inp['kern']), dev(inp['uv']), dev(inp['w_plane']), dev(inp['weights'])
    if precision == 'f32':
        runs = [('generic', 'fp32'), ('binned', 'fp32')] + [('mfma', a) for a in eg.DEGRID_FORMS]
    else:
        runs = [('generic', None), ('mfma', None), ('binned', None)]
    for variant, arith in runs:
        cdt = np.complex64 if precision == 'f32' else np.complex128
        g = padded(inp['grid'].astype(cdt), layout, 0, origin=(1, 1))      # (a sub-image pointer in both)
        vis = dev(inp['vis'])
        if variant == 'binned':
            ws, nbytes = gridder_workspace(L().kimg_degrid_binned_workspace_bytes, n, P, W, OV, K)
        else:
            ws, nbytes = gridder_workspace(L().kimg_degrid_workspace_bytes, P, W, OV, K)
        head = (g.ptr, g.row, g.pol, G, P, uv.ptr, wp.ptr, weights.ptr, vis.ptr, n, table.ptr, W, OV, K,
                ws.ptr, nbytes, kgrid.GRID_VARIANTS[variant])
        if precision == 'f32':
            ok(L().kimg_degrid(*head, kgrid.GRID_ARITH[arith], q.handle))
        else:
            ok(L().kimg_degrid_f64(*head, q.handle))
        q.finish()
        eg._assert_exact(vis.get(q), want, '%s/%s' % (variant, arith))
        np.testing.assert_array_equal(g.get(q), inp['grid'].astype(cdt))


# ---------------------------------------------------------------------------------------------
# CLEAN (square: orc.Clean is)

FORMS = {'auto': 0, 'two_launch': 1, 'one_launch': 2}
CLEAN_CASES = [(0, 1, 0), (1, 2, 1), (2, 4, 0), (3, 4, 1)]      # (seed, P, mode)
PATCH = (33, 47)


def clean_problem(seed, P, mode):
    """The input generator of test_hip_parity.test_clean_fuzz (Gaussian PSF with noise, noise
    with ten spikes), with P and mode given, a border > 0, and spikes next to the image edge
    whose patches are clipped."""
    rs = np.random.RandomState(5000 + seed)
    G = int(rs.choice([96, 144, 200, 256]))
    border = float(rs.choice([0.02, 0.05]))
    loop_gain = float(rs.choice([0.05, 0.1, 0.5]))
    g1 = np.exp(-0.5 * ((np.arange(G) - G // 2) / rs.uniform(1.5, 8.0)) ** 2)
    psf = np.empty((P, G, G), np.float32)
    for p in range(P):
        psf[p] = np.outer(g1, g1) + 0.01 * rs.standard_normal((G, G))
    psf /= psf[:, G // 2, G // 2][:, None, None]
    dirty = (0.3 * rs.standard_normal((P, G, G))).astype(np.float32)
    for _ in range(10):
        y, x = rs.randint(0, G, 2)
        dirty[:, y, x] += rs.uniform(2.0, 10.0, P).astype(np.float32) * rs.choice([-1, 1])
    bp = round(G * border)
    for y, x, amp in ((bp + 1, G // 2, 12.0), (G // 3, G - bp - 1, -11.0)):
        dirty[:, y, x] += np.float32(amp)
    return G, border, loop_gain, psf, dirty


class CleanBuffers:
    """dirty and model in one padded layout (the ABI gives them one stride pair), the PSF in
    another, a mask with mask_row_stride = width + 5; dense tile arrays, state and log."""

    def __init__(self, G, border, psf, dirty, layout, mask=None, cycles=1):
        ctx, q = context_queue()
        self.q = q
        P = dirty.shape[0]
        self.P, self.G, self.bp = P, G, round(G * border)
        self.dirty = padded(dirty, layout, 0)
        self.model = padded(np.zeros_like(dirty), layout, 0)
        self.psf = padded(psf, layout, 1)
        self.mask = None if mask is None else Padded(ctx, q, mask, rpad=5, vpad=1)
        self.tiles = -(-(G - 2 * self.bp) // 32)
        self.tile_max = dev(np.full((self.tiles, self.tiles), 7.0, np.float32))
        self.tile_pos = dev(np.full((self.tiles, self.tiles, 2), 7, np.int32))
        self.state = dev(np.zeros(L().kimg_clean_state_bytes(P, self.tiles, self.tiles) // 4, np.int32))
        self.log = dev(np.zeros((cycles, 3 + P), np.float32))

    def image(self):
        return (self.dirty.ptr, self.dirty.row, self.dirty.pol, self.G, self.G, self.P)

    def psf_args(self):
        return (self.psf.ptr, self.psf.row, self.psf.pol, self.G, self.G)

    def mask_args(self):
        return (self.mask.ptr, self.mask.row)

    def update_tiles(self, mode, tx0, ty0, tx1, ty1):
        args = (*self.image(), self.bp, mode, self.tile_max.ptr, self.tile_pos.ptr, self.tiles, self.tiles,
                tx0, ty0, tx1, ty1, self.q.handle)
        if self.mask is None:
            ok(L().kimg_update_tiles(*args))
        else:
            ok(L().kimg_update_tiles_masked(*args, *self.mask_args()))

    def reset(self, mode):
        self.update_tiles(mode, 0, 0, self.tiles, self.tiles)

    def collect(self):
        """(log as the reference returns it, dirty, model, tile_max, tile_pos); the padding of
        every strided array checked."""
        q = self.q
        q.finish()
        state = self.state.get(q)
        assert state[1] != 2
        log = self.log.get(q)[:int(state[0])]
        rows = [(r[0], tuple(int(v) for v in r[1:3].view(np.int32)), r[3:].copy()) for r in log]
        self.psf.get(q)
        if self.mask is not None:
            self.mask.get(q)
        return rows, self.dirty.get(q), self.model.get(q), self.tile_max.get(q), self.tile_pos.get(q)


def clean_truth(G, border, loop_gain, mode, dirty, psf, patch, threshold, cycles, mask=None):
    from test_clean_mask import masked_run, plain_run
    if mask is None:
        return plain_run(G, border, loop_gain, mode, dirty, psf, patch, threshold, cycles)
    return masked_run(G, border, loop_gain, mode, dirty, psf, patch, threshold, cycles, mask)


def clean_mask(G, border):
    """Half of the pixels allowed at random, among them the two spikes next to the edge."""
    rs = np.random.RandomState(G)
    mask = (rs.uniform(size=(G, G)) < 0.5).astype(np.uint8)
    bp = round(G * border)
    mask[bp + 1, G // 2] = mask[G // 3, G - bp - 1] = 1
    return mask


def clipped(rows, G, patch):
    return [pos for _, pos, _ in rows if pos[0] < patch[1] // 2 or pos[1] < patch[2] // 2
            or pos[0] >= G - patch[1] // 2 or pos[1] >= G - patch[2] // 2]


@gpu
@layouts
@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('seed,P,mode', CLEAN_CASES)
def test_clean_steps(seed, P, mode, masked, layout):
    """kimg_update_tiles, kimg_find_peak and kimg_subtract_psf (and the masked pair) one cycle at
    a time, as the per-call path drives them, against orc.Clean / the masked restatement of
    tests/test_clean_mask.py: peak value, position, pixel, dirty, model and tile arrays bit for
    bit after every cycle batch; at least one patch is clipped at the image edge."""
    from test_clean_mask import same_run
    G, border, loop_gain, psf, dirty = clean_problem(seed, P, mode)
    patch = (P,) + PATCH
    mask = clean_mask(G, border) if masked else None
    cycles = 12
    want = clean_truth(G, border, loop_gain, mode, dirty, psf, patch, 0.0, cycles, mask)
    assert len(want[0]) == cycles and clipped(want[0], G, patch)
    b = CleanBuffers(G, border, psf, dirty, layout, mask)
    q = b.q
    b.reset(mode)
    peak_value = guarded(np.zeros(1, np.float32), 1)
    peak_pos = guarded(np.zeros(2, np.int32), 1, np.int32)
    peak_pixel = dev(np.zeros(P, np.float32))
    rows = []
    for _ in range(cycles):
        args = (b.dirty.ptr, b.dirty.row, b.dirty.pol, P, b.tile_max.ptr, b.tile_pos.ptr, b.tiles, b.tiles,
                peak_value.ptr, peak_pos.ptr, peak_pixel.ptr, q.handle)
        ok(L().kimg_find_peak_masked(*args, *b.mask_args()) if masked else L().kimg_find_peak(*args))
        value = peak_value.get(q)[0, 0, 0]
        y, x = (int(v) for v in peak_pos.get(q)[0, 0])
        pixel = peak_pixel.get(q)
        rows.append((value, (y, x), np.float32(loop_gain) * pixel))
        ok(L().kimg_subtract_psf(b.dirty.ptr, b.model.ptr, b.dirty.row, b.dirty.pol, G, G, P, *b.psf_args(),
                                 patch[2], patch[1], peak_pixel.ptr, x, y, loop_gain, q.handle))
        x0, y0 = max(x - patch[2] // 2, 0), max(y - patch[1] // 2, 0)
        x1, y1 = min(x - patch[2] // 2 + patch[2], G), min(y - patch[1] // 2 + patch[1], G)
        b.update_tiles(mode, max((x0 - b.bp) // 32, 0), max((y0 - b.bp) // 32, 0),
                       min(-(-(x1 - b.bp) // 32), b.tiles), min(-(-(y1 - b.bp) // 32), b.tiles))
    q.finish()
    b.psf.get(q)
    same_run((rows, b.dirty.get(q), b.model.get(q), b.tile_max.get(q), b.tile_pos.get(q)), want)


@gpu
@layouts
@pytest.mark.parametrize('seed,P,mode', CLEAN_CASES)
def test_clean_loops(seed, P, mode, layout):
    """The device-resident loops on padded layouts, bit for bit against orc.Clean (and the masked
    restatement): kimg_clean_cycles as two_launch, one_launch and auto (which takes the
    multi-component form here: checked, and compared with oracle/clean_multi_model.py as well),
    kimg_clean_cycles_masked in both of its forms, kimg_clean_major_cycles with the threshold the
    frontend would make, kimg_clean_cycles_batch with two channels of different patches."""
    from test_clean_mask import same_run
    from katsdpimager_amd import clean
    from katsdpimager_amd._lib import CleanChannel
    from oracle.clean_multi_model import MultiClean
    G, border, loop_gain, psf, dirty = clean_problem(seed, P, mode)
    patch = (P,) + PATCH
    cycles = 60
    first = clean_truth(G, border, loop_gain, mode, dirty, psf, patch, 0.0, 1)[0][0][0]
    threshold = 0.05 * float(first)
    want = clean_truth(G, border, loop_gain, mode, dirty, psf, patch, threshold, cycles)
    assert clipped(want[0], G, patch) and len(want[0]) > 3

    def loop_args(b, threshold, cycles, form):
        return (b.dirty.ptr, b.model.ptr, b.dirty.row, b.dirty.pol, G, G, P, *b.psf_args(), patch[2], patch[1],
                b.bp, mode, loop_gain, threshold, b.tile_max.ptr, b.tile_pos.ptr, b.tiles, b.tiles, cycles,
                form, b.state.ptr, b.log.ptr, b.q.handle)

    for form in FORMS:
        b = CleanBuffers(G, border, psf, dirty, layout, cycles=cycles)
        b.reset(mode)
        ok(L().kimg_clean_cycles(*loop_args(b, threshold, cycles, FORMS[form])))
        same_run(b.collect(), want)
        took_multi = int(b.state.get(b.q)[4]) == 0x4d554c54         # (clean.Clean.last_launches)
        assert took_multi == (form == 'auto'), form
        if took_multi:
            # ... whose executable specification is oracle/clean_multi_model.py
            img, model = dirty.copy(), np.zeros_like(dirty)
            mc = MultiClean(G, border, loop_gain, mode, img, psf, model, patch, threshold, cycles)
            rows = mc.run()
            same_run(b.collect(), (rows, img, model, mc.tile_max.reshape(want[3].shape),
                                   mc.tile_pos.reshape(want[4].shape)))

    mask = clean_mask(G, border)
    want_masked = clean_truth(G, border, loop_gain, mode, dirty, psf, patch, threshold, cycles, mask)
    assert len(want_masked[0]) > 3
    for form in ('two_launch', 'one_launch'):
        b = CleanBuffers(G, border, psf, dirty, layout, mask, cycles=cycles)
        b.reset(mode)
        ok(L().kimg_clean_cycles_masked(*loop_args(b, threshold, cycles, FORMS[form]), *b.mask_args()))
        same_run(b.collect(), want_masked)

    # one major cycle: the threshold as frontend.py:568-575 makes it from the first peak
    peak_power = clean.metric_to_power(mode, float(first))
    noise_threshold, left = 1e-4 * peak_power, 0.15
    metric = float(np.float32(clean.power_to_metric(mode, max(noise_threshold, left * peak_power))))
    major = clean_truth(G, border, loop_gain, mode, dirty, psf, patch, metric, cycles)
    assert 1 < len(major[0])
    b = CleanBuffers(G, border, psf, dirty, layout, cycles=cycles)
    b.reset(mode)
    done, first_peak = ctypes.c_int(0), ctypes.c_float(0.0)
    args = loop_args(b, None, cycles, 0)
    ok(L().kimg_clean_major_cycles(*args[:17], noise_threshold, left, *args[18:], ctypes.byref(done),
                                   ctypes.byref(first_peak)))
    same_run(b.collect(), major)
    assert done.value == len(major[0]) and first_peak.value == first

    # two channels in one batch: the second with its own image, patch, threshold and cycle limit
    dirty2 = (dirty[:, ::-1, :] * np.float32(0.75)).copy()
    patch2 = (P, 21, 35)
    want2 = clean_truth(G, border, loop_gain, mode, dirty2, psf, patch2, 0.0, 25)
    bs = [CleanBuffers(G, border, psf, dirty, layout, cycles=cycles),
          CleanBuffers(G, border, psf, dirty2, layout, cycles=cycles)]
    assert (bs[0].dirty.row, bs[0].dirty.pol, bs[0].psf.row) == (bs[1].dirty.row, bs[1].dirty.pol, bs[1].psf.row)
    channels = (CleanChannel * 2)()
    for c, (b, pt, th, n) in enumerate(zip(bs, (patch, patch2), (threshold, 0.0), (cycles, 25))):
        b.reset(mode)
        channels[c] = CleanChannel(b.dirty.ptr, b.model.ptr, b.psf.ptr, b.tile_max.ptr, b.tile_pos.ptr,
                                   b.state.ptr, b.log.ptr, pt[2], pt[1], th, n)
    b = bs[0]
    ok(L().kimg_clean_cycles_batch(channels, 2, b.dirty.row, b.dirty.pol, G, G, P, b.psf.row, b.psf.pol, G, G,
                                   b.bp, mode, loop_gain, b.tiles, b.tiles, b.q.handle))
    same_run(bs[0].collect(), want)
    same_run(bs[1].collect(), want2)


# ---------------------------------------------------------------------------------------------
# argument checks: a row stride below the width is KIMG_EINVAL and nothing is launched

def _refusals(bad=63):
    """name -> function(buffers) -> status.  `S` is a float32 Padded of sentinels with interior
    [4][64][64] (viewed as whatever the call takes), `X` a dense scratch array; the width is 64
    and the stride under test 63."""
    W = H = 64
    one = ctypes.c_float * 4
    one64 = ctypes.c_double * 4

    def img(S, row=bad):
        return (S.ptr, row, S.pol, W, H, 1)

    def loop(S, X, row, psf_row, extra=()):
        return (S.ptr, S.ptr, row, S.pol, W, H, 1, S.ptr, psf_row, S.pol, W, H, 9, 9, 2, 0, 0.1, *extra)

    tail = lambda X: (X.ptr, X.ptr, 2, 2)       # noqa: E731  (tile_max, tile_pos, tiles_x, tiles_y)
    ws = 1 << 20
    return {
        'kimg_grid': lambda S, X: L().kimg_grid(S.ptr, bad, S.pol, W, 1, S.ptr, W, S.pol, X.ptr, X.ptr, X.ptr, 4,
                                                X.ptr, 1, 1, 7, X.ptr, ws, 0, 0, None),
        'kimg_grid weights_grid': lambda S, X: L().kimg_grid(S.ptr, W, S.pol, W, 1, S.ptr, bad, S.pol, X.ptr,
                                                             X.ptr, X.ptr, 4, X.ptr, 1, 1, 7, X.ptr, ws, 0, 0, None),
        'kimg_grid_f64': lambda S, X: L().kimg_grid_f64(S.ptr, bad, S.pol, W, 1, S.ptr, W, S.pol, X.ptr, X.ptr,
                                                        X.ptr, 4, X.ptr, 1, 1, 7, X.ptr, ws, 0, None),
        'kimg_degrid': lambda S, X: L().kimg_degrid(S.ptr, bad, S.pol, W, 1, X.ptr, X.ptr, X.ptr, X.ptr, 4, X.ptr,
                                                    1, 1, 7, X.ptr, ws, 0, 0, None),
        'kimg_degrid_f64': lambda S, X: L().kimg_degrid_f64(S.ptr, bad, S.pol, W, 1, X.ptr, X.ptr, X.ptr, X.ptr, 4,
                                                            X.ptr, 1, 1, 7, X.ptr, ws, 0, None),
        'kimg_grid_weights': lambda S, X: L().kimg_grid_weights(*img(S), X.ptr, X.ptr, 4, None),
        'kimg_mean_weight': lambda S, X: L().kimg_mean_weight(X.ptr, S.ptr, bad, W, H, None),
        'kimg_density_weights': lambda S, X: L().kimg_density_weights(X.ptr, *img(S), 1.0, 1.0, None),
        'kimg_density_weights_robust': lambda S, X: L().kimg_density_weights_robust(X.ptr, *img(S), X.ptr, 1.0,
                                                                                    1.0, None),
        'kimg_grid_to_layer': lambda S, X: L().kimg_grid_to_layer(X.ptr, W, S.ptr, bad, W, None),
        'kimg_layer_to_grid': lambda S, X: L().kimg_layer_to_grid(S.ptr, bad, W, X.ptr, W, None),
        'kimg_grid_to_layer_f64': lambda S, X: L().kimg_grid_to_layer_f64(X.ptr, W, S.ptr, bad, W, None),
        'kimg_layer_to_grid_f64': lambda S, X: L().kimg_layer_to_grid_f64(S.ptr, bad, W, X.ptr, W, None),
        'kimg_grid_to_half_layer': lambda S, X: L().kimg_grid_to_half_layer(X.ptr, W, S.ptr, bad, W, None),
        'kimg_half_layer_to_grid': lambda S, X: L().kimg_half_layer_to_grid(S.ptr, bad, W, X.ptr, W, None),
        'kimg_layer_to_image': lambda S, X: L().kimg_layer_to_image(S.ptr, bad, X.ptr, W, X.ptr, 0.0, 0.0, 0.0, None),
        'kimg_image_to_layer': lambda S, X: L().kimg_image_to_layer(X.ptr, S.ptr, bad, W, X.ptr, 0.0, 0.0, 0.0, None),
        'kimg_layer_to_image_f64': lambda S, X: L().kimg_layer_to_image_f64(S.ptr, bad, X.ptr, W, X.ptr, 0.0, 0.0,
                                                                            0.0, None),
        'kimg_image_to_layer_f64': lambda S, X: L().kimg_image_to_layer_f64(X.ptr, S.ptr, bad, W, X.ptr, 0.0, 0.0,
                                                                            0.0, None),
        'kimg_real_layer_to_image': lambda S, X: L().kimg_real_layer_to_image(S.ptr, bad, X.ptr, W, W, X.ptr, 0.0,
                                                                              0.0, None),
        'kimg_real_layer_to_image layer': lambda S, X: L().kimg_real_layer_to_image(X.ptr, W, S.ptr, bad, W, X.ptr,
                                                                                    0.0, 0.0, None),
        'kimg_image_to_real_layer': lambda S, X: L().kimg_image_to_real_layer(X.ptr, W, S.ptr, bad, W, X.ptr, 0.0,
                                                                              0.0, None),
        'kimg_image_to_real_layer layer': lambda S, X: L().kimg_image_to_real_layer(S.ptr, bad, X.ptr, W, W, X.ptr,
                                                                                    0.0, 0.0, None),
        'kimg_grid_to_image_real': lambda S, X: L().kimg_grid_to_image_real(S.ptr, bad, W, X.ptr, W, W, X.ptr, 0.0,
                                                                            0.0, 0, X.ptr, ws, None),
        'kimg_grid_to_image_real grid': lambda S, X: L().kimg_grid_to_image_real(X.ptr, W, W, S.ptr, bad, W, X.ptr,
                                                                                 0.0, 0.0, 0, X.ptr, ws, None),
        'kimg_image_to_grid_real': lambda S, X: L().kimg_image_to_grid_real(S.ptr, bad, W, X.ptr, W, W, X.ptr, 0.0,
                                                                            0.0, X.ptr, ws, None),
        'kimg_image_to_grid_real image': lambda S, X: L().kimg_image_to_grid_real(X.ptr, W, W, S.ptr, bad, W, X.ptr,
                                                                                  0.0, 0.0, X.ptr, ws, None),
        'kimg_grid_to_image_w': lambda S, X: L().kimg_grid_to_image_w(S.ptr, bad, W, X.ptr, W, W, X.ptr, 0.0, 0.0,
                                                                      1.0, 0, X.ptr, ws, None),
        'kimg_image_to_grid_w': lambda S, X: L().kimg_image_to_grid_w(S.ptr, bad, W, X.ptr, W, W, X.ptr, 0.0, 0.0,
                                                                      1.0, X.ptr, ws, None),
        'kimg_convolve_beam': lambda S, X: L().kimg_convolve_beam(S.ptr, bad, W, 1.0, 0.0, 0.0, 0.0, X.ptr, ws, None),
        'kimg_fourier_beam': lambda S, X: L().kimg_fourier_beam(S.ptr, bad, W, H, 1.0, 0.0, 0.0, 0.0, None),
        'kimg_scale': lambda S, X: L().kimg_scale(*img(S), one(1, 1, 1, 1), None),
        'kimg_scale_f64': lambda S, X: L().kimg_scale_f64(*img(S), one64(1, 1, 1, 1), None),
        'kimg_scale_device': lambda S, X: L().kimg_scale_device(*img(S), X.ptr, None),
        'kimg_pixel_reciprocal': lambda S, X: L().kimg_pixel_reciprocal(*img(S), 1, 1, X.ptr, None),
        'kimg_add_image dest': lambda S, X: L().kimg_add_image(S.ptr, bad, S.pol, X.ptr, W, W * H, W, H, 1, None),
        'kimg_add_image src': lambda S, X: L().kimg_add_image(S.ptr, S.row, S.pol, X.ptr, bad, W * H, W, H, 1, None),
        'kimg_add_image_f64': lambda S, X: L().kimg_add_image_f64(S.ptr, bad, S.pol, X.ptr, W, W * H, W, H, 1, None),
        'kimg_apply_primary_beam': lambda S, X: L().kimg_apply_primary_beam(S.ptr, bad, S.pol, X.ptr, W, W, H, 1,
                                                                            0.5, 0.0, None),
        'kimg_apply_primary_beam beam': lambda S, X: L().kimg_apply_primary_beam(S.ptr, S.row, S.pol, X.ptr, bad,
                                                                                 W, H, 1, 0.5, 0.0, None),
        'kimg_apply_primary_beam_f64': lambda S, X: L().kimg_apply_primary_beam_f64(S.ptr, bad, S.pol, X.ptr, W, W,
                                                                                    H, 1, 0.5, 0.0, None),
        'kimg_image_peak': lambda S, X: L().kimg_image_peak(S.ptr, bad, S.pol, None, 0, W, H, 1, 1.0, X.ptr, None),
        'kimg_image_peak beam': lambda S, X: L().kimg_image_peak(S.ptr, S.row, S.pol, X.ptr, bad, W, H, 1, 1.0, X.ptr,
                                                                 None),
        'kimg_image_nansum': lambda S, X: L().kimg_image_nansum(*img(S), X.ptr, None),
        # (no width in this call: the region must fit a row)
        'kimg_psf_patch': lambda S, X: L().kimg_psf_patch(S.ptr, bad, S.pol, 1, 0, 0, W - 1, H - 1, 32, 32, 0.5,
                                                          X.ptr, None),
        'kimg_abs_histogram': lambda S, X: L().kimg_abs_histogram(*img(S), 2, 3, 0, X.ptr, None),
        'kimg_abs_count_le': lambda S, X: L().kimg_abs_count_le(*img(S), 2, 1.0, X.ptr, None),
        'kimg_noise_est': lambda S, X: L().kimg_noise_est(*img(S), 2, 1.0, X.ptr, X.ptr, None),
        'kimg_update_tiles': lambda S, X: L().kimg_update_tiles(*img(S), 2, 0, X.ptr, X.ptr, 2, 2, 0, 0, 2, 2, None),
        'kimg_update_tiles_masked': lambda S, X: L().kimg_update_tiles_masked(
            *img(S), 2, 0, X.ptr, X.ptr, 2, 2, 0, 0, 2, 2, None, X.ptr, W),
        'kimg_update_tiles_masked mask': lambda S, X: L().kimg_update_tiles_masked(
            *img(S, S.row), 2, 0, X.ptr, X.ptr, 2, 2, 0, 0, 2, 2, None, X.ptr, bad),
        'kimg_subtract_psf': lambda S, X: L().kimg_subtract_psf(S.ptr, S.ptr, bad, S.pol, W, H, 1, S.ptr, S.row,
                                                                S.pol, W, H, 9, 9, X.ptr, 30, 30, 0.1, None),
        'kimg_subtract_psf psf': lambda S, X: L().kimg_subtract_psf(S.ptr, S.ptr, S.row, S.pol, W, H, 1, S.ptr, bad,
                                                                    S.pol, W, H, 9, 9, X.ptr, 30, 30, 0.1, None),
        'kimg_clean_cycles': lambda S, X: L().kimg_clean_cycles(*loop(S, X, bad, S.row, (0.0,)), *tail(X), 5, 1,
                                                                X.ptr, X.ptr, None),
        'kimg_clean_cycles psf': lambda S, X: L().kimg_clean_cycles(*loop(S, X, S.row, bad, (0.0,)), *tail(X), 5, 1,
                                                                    X.ptr, X.ptr, None),
        'kimg_clean_cycles_masked': lambda S, X: L().kimg_clean_cycles_masked(
            *loop(S, X, bad, S.row, (0.0,)), *tail(X), 5, 1, X.ptr, X.ptr, None, X.ptr, W),
        'kimg_clean_cycles_masked mask': lambda S, X: L().kimg_clean_cycles_masked(
            *loop(S, X, S.row, S.row, (0.0,)), *tail(X), 5, 1, X.ptr, X.ptr, None, X.ptr, bad),
        'kimg_clean_major_cycles': lambda S, X: L().kimg_clean_major_cycles(
            *loop(S, X, bad, S.row, (0.0, 0.5)), *tail(X), 5, 0, X.ptr, X.ptr, None, None, None),
        'kimg_clean_cycles_batch': lambda S, X: _batch(S, X, bad, S.row),
        'kimg_clean_cycles_batch psf': lambda S, X: _batch(S, X, S.row, bad),
    }


def _batch(S, X, row, psf_row):
    from katsdpimager_amd._lib import CleanChannel
    channels = (CleanChannel * 1)(CleanChannel(S.ptr, S.ptr, S.ptr, X.ptr, X.ptr, X.ptr, X.ptr, 9, 9, 0.0, 5))
    return L().kimg_clean_cycles_batch(channels, 1, row, S.pol, 64, 64, 1, psf_row, S.pol, 64, 64, 2, 0, 0.1,
                                       2, 2, None)


REFUSALS = sorted(_refusals())


@gpu
@pytest.mark.parametrize('name', REFUSALS)
def test_stride_below_width_is_refused(name):
    """row_stride = width - 1 (of each strided array of the call in turn) is KIMG_EINVAL before
    anything is enqueued: the image buffer -- sentinels inside and out -- and the scratch array
    every other pointer of the call points at come back bit for bit."""
    ctx, q = context_queue()
    S = Padded(ctx, q, np.full((4, 64, 64), -3.0e38, np.float32), rpad=3, vpad=2, origin=(1, 1))
    scratch = np.full(1 << 18, 1.0e30, np.float32)
    X = dev(scratch)
    q.finish()
    assert _refusals()[name](S, X) == KIMG_EINVAL
    import torch
    torch.cuda.synchronize()
    assert np.all(S.get(q) == np.float32(-3.0e38))
    np.testing.assert_array_equal(X.get(q), scratch)


def strided_entry_points_without_refusal():
    """Functions of include/kimg.h with a *_stride parameter that have no refusal case."""
    import re
    text = open(os.path.join(ROOT, 'include', 'kimg.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    strided = {m.group(1) for m in re.finditer(r'\bint\s+(kimg_\w+)\s*\(([^;]*?)\)\s*;', text, flags=re.S)
               if '_stride' in m.group(2)}
    assert len(strided) > 40
    covered = {name.split()[0] for name in REFUSALS}
    return strided - covered
