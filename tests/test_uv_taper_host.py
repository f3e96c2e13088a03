"""The uv taper's host side (weight.UVTaperParameters, weight.uv_taper_host): the numpy statement
of what kimg_density_weights_taper computes per cell (include/kimg.h), its validation, and the
position-angle convention against beam.fit_beam.  No GPU."""
import math

import numpy as np
import pytest

from katsdpimager_amd import beam, parameters
from katsdpimager_amd.weight import UVTaperParameters, WeightType, uv_taper_host

K = math.pi ** 2 / (4.0 * math.log(2.0))


def cell_uv(shape, image_size):
    H, W = shape
    u = (np.arange(W) - W // 2) / image_size
    v = (np.arange(H) - H // 2) / image_size
    return u[None, :], v[:, None]


def test_origin_and_symmetry():
    """T = 1 at the origin cell (W/2, H/2), and T(-u, -v) = T(u, v) wherever both cells exist
    (row 0 and column 0 have no mirror image on an even grid)."""
    p = UVTaperParameters((3e-3, 1e-3, 0.7), max_uv=900.0, outer_tukey=300.0)
    H, W = 40, 64
    t = uv_taper_host((H, W), 0.05, p)
    assert t.shape == (H, W) and t.dtype == np.float64
    assert t[H // 2, W // 2] == 1.0
    np.testing.assert_array_equal(t[1:, 1:], t[1:, 1:][::-1, ::-1])
    assert np.all((t >= 0) & (t <= 1))
    # a leading polarization axis in `shape` is ignored
    np.testing.assert_array_equal(uv_taper_host((4, H, W), 0.05, p), t)


def test_identity():
    t = uv_taper_host((6, 10), 0.01, UVTaperParameters())
    np.testing.assert_array_equal(t, np.ones((6, 10)))


def test_circular_closed_form():
    """One FWHM: G = exp(-(pi^2 / (4 ln 2)) fwhm^2 r^2), and half power in the uv plane at
    r = 2 ln 2 / (pi fwhm) ... to rounding (a few ulp of the exponent)."""
    fwhm, image_size = 2.5e-3, 0.04
    shape = (48, 36)
    u, v = cell_uv(shape, image_size)
    t = uv_taper_host(shape, image_size, UVTaperParameters(fwhm))
    np.testing.assert_allclose(t, np.exp(-K * fwhm ** 2 * (u * u + v * v)), rtol=1e-13, atol=0)
    assert UVTaperParameters(fwhm) == UVTaperParameters((fwhm, fwhm, 0.0))
    # the scalar the definition gives at one cell
    x, y = 23, 30
    r2 = ((x - 18) / image_size) ** 2 + ((y - 24) / image_size) ** 2
    assert t[y, x] == pytest.approx(math.exp(-K * fwhm ** 2 * r2), rel=1e-13)


def test_elliptical_axes():
    """Position angle 0: the major axis lies along axis 0 (v); pi/2: along axis 1 (u)."""
    major, minor, image_size = 4e-3, 1e-3, 0.05
    shape = (32, 32)
    u, v = cell_uv(shape, image_size)
    t0 = uv_taper_host(shape, image_size, UVTaperParameters((major, minor, 0.0)))
    np.testing.assert_allclose(t0, np.exp(-K * (major ** 2 * v * v + minor ** 2 * u * u)), rtol=1e-13)
    t90 = uv_taper_host(shape, image_size, UVTaperParameters((major, minor, math.pi / 2)))
    np.testing.assert_allclose(t90, np.exp(-K * (major ** 2 * u * u + minor ** 2 * v * v)), rtol=1e-12)


def test_cuts_and_ramps():
    """image_size 1: cell (x, y) stands at integer (u, v).  Cuts: 0 strictly inside min_uv and
    strictly outside max_uv, 1 on the radii themselves.  Ramps: 0 at min_uv, 0.5 half way, 1 from
    min_uv + inner_tukey on, and the mirror image below max_uv."""
    shape = (64, 64)
    c = 32

    def at(t, r):               # the cell at (u, v) = (r, 0)
        return t[c, c + r]

    t = uv_taper_host(shape, 1.0, UVTaperParameters(min_uv=4.0, max_uv=20.0))
    assert [at(t, r) for r in (0, 3, 4, 5, 19, 20, 21, 30)] == [0, 0, 1, 1, 1, 1, 0, 0]
    assert t[c + 3, c + 3] == 1 and t[c + 2, c + 2] == 0        # r = 4.24, 2.83
    assert t[c + 14, c + 14] == 1 and t[c + 15, c + 15] == 0    # r = 19.8, 21.2
    t = uv_taper_host(shape, 1.0, UVTaperParameters(min_uv=4.0, max_uv=24.0, inner_tukey=6.0,
                                                    outer_tukey=8.0))
    assert at(t, 3) == 0 and at(t, 4) == 0
    assert at(t, 7) == pytest.approx(0.5, rel=1e-15)
    assert at(t, 5) == pytest.approx(0.5 * (1 - math.cos(math.pi / 6)), rel=1e-14)
    assert at(t, 10) == 1 and at(t, 12) == 1 and at(t, 16) == 1
    assert at(t, 20) == pytest.approx(0.5, rel=1e-15)
    assert at(t, 22) == pytest.approx(0.5 * (1 - math.cos(math.pi / 4)), rel=1e-14)
    assert at(t, 24) == 0 and at(t, 25) == 0
    # an inner ramp without a cut starts at the origin
    t = uv_taper_host(shape, 1.0, UVTaperParameters(inner_tukey=10.0))
    assert at(t, 0) == 0 and at(t, 5) == pytest.approx(0.5, rel=1e-15) and at(t, 10) == 1
    # all factors multiply
    g = UVTaperParameters(0.02, min_uv=4.0, max_uv=24.0, inner_tukey=6.0, outer_tukey=8.0)
    t = uv_taper_host(shape, 1.0, g)
    assert at(t, 7) == pytest.approx(0.5 * math.exp(-K * 0.02 ** 2 * 49), rel=1e-14)


@pytest.mark.parametrize('kwargs', [
    dict(gaussian=-1.0), dict(gaussian=float('nan')), dict(gaussian=float('inf')),
    dict(gaussian=(1e-3, 2e-3, 0.0)), dict(gaussian=(2e-3, 1e-3, float('nan'))),
    dict(gaussian=(2e-3, -1e-3, 0.0)), dict(gaussian=(2e-3, 1e-3)),
    dict(min_uv=-1.0), dict(max_uv=float('nan')), dict(min_uv=float('inf')),
    dict(min_uv=10.0, max_uv=10.0), dict(min_uv=11.0, max_uv=10.0),
    dict(inner_tukey=-1.0), dict(outer_tukey=float('inf'), max_uv=10.0),
    dict(min_uv=2.0, max_uv=10.0, inner_tukey=5.0, outer_tukey=4.0),
    dict(max_uv=10.0, inner_tukey=11.0), dict(outer_tukey=3.0),
])
def test_validation(kwargs):
    with pytest.raises(ValueError):
        UVTaperParameters(**kwargs)


def test_valid_edge_cases():
    UVTaperParameters(min_uv=2.0, max_uv=10.0, inner_tukey=4.0, outer_tukey=4.0)     # ramps that touch
    UVTaperParameters((2e-3, 2e-3, 0.3))
    UVTaperParameters(0.0)


def test_from_arcsec_and_equality():
    a = UVTaperParameters.from_arcsec(30.0)
    rad = math.radians(30.0 / 3600.0)
    assert a.gaussian == pytest.approx((rad, rad, 0.0), rel=1e-15)
    b = UVTaperParameters.from_arcsec((30.0, 20.0), 30.0, max_uv=5000.0, outer_tukey=100.0)
    assert b.gaussian == pytest.approx((rad, math.radians(20.0 / 3600.0), math.radians(30.0)), rel=1e-15)
    assert b.max_uv == 5000.0 and b.outer_tukey == 100.0
    assert a != b and a == UVTaperParameters.from_arcsec(30.0)
    assert hash(a) == hash(UVTaperParameters(a.gaussian[0]))
    assert UVTaperParameters.from_arcsec(min_uv=3.0).gaussian is None
    assert 'max_uv=5000.0' in repr(b)


def test_weight_parameters_carry_the_taper():
    wp = parameters.WeightParameters(WeightType.ROBUST, 0.5)
    assert wp.taper is None and wp.robustness == 0.5
    t = UVTaperParameters(1e-3)
    assert parameters.WeightParameters(WeightType.NATURAL, taper=t).taper is t


def test_coefficients_are_the_c_struct():
    """The seven doubles of kimg_uv_taper: no cut is min_uv = 0 and the largest double (every
    field of the struct must be finite)."""
    import sys
    assert UVTaperParameters().coefficients() == (0.0, 0.0, 0.0, 0.0, sys.float_info.max, 0.0, 0.0)
    major, minor, pa = 3e-3, 1e-3, math.radians(30)
    q = UVTaperParameters((major, minor, pa), 5.0, 90.0, 2.0, 3.0).coefficients()
    c, s = math.cos(pa), math.sin(pa)
    assert q[0] == pytest.approx(K * (major ** 2 * s * s + minor ** 2 * c * c), rel=1e-15)
    assert q[1] == pytest.approx(2 * K * (major ** 2 - minor ** 2) * s * c, rel=1e-15)
    assert q[2] == pytest.approx(K * (major ** 2 * c * c + minor ** 2 * s * s), rel=1e-15)
    assert q[3:] == (5.0, 90.0, 2.0, 3.0)


def test_position_angle_is_fit_beams():
    """The float64 inverse DFT of an elliptical G at 30 degrees is a Gaussian beam for which
    beam.fit_beam returns the major and minor FWHM and the position angle that were asked for (a
    transposed convention would give 60 degrees, a mirrored one 150).

    Grid 128 x 128, image_size S, pixel S / 128, FWHM 9 and 5 pixels.

    Tolerance.  fit_beam fits a Gaussian to samples at the pixels themselves, so an exact Gaussian
    is fitted without any sampling error: what remains is how far the DFT's image is from the
    Gaussian, delta per pixel in units of the peak.
      * Truncation of G at the grid edge.  In cell units G <= exp(-a r^2) with a = K (5 / 128)^2 =
        5.43e-3, so the mass outside the grid (r >= 64) is at most (pi / a) exp(-a 64^2) =
        579 * 2.2e-10 = 1.3e-7, against a total mass of pi / (K * 9 * 5 / 128^2) = 321:
        delta <= 4e-10 at every pixel.
      * Periodic images of the beam stand 128 pixels away: exp(-4 ln 2 (108 / 9)^2) < 1e-170.
      * Rounding of the DFT: 1e-15.
    The fit is a linear-ised least-squares problem over the n ~ 300 samples above 0.01; its
    Jacobian columns (d model / d ln sigma, d model / d theta) have rms >= 0.05 over those samples,
    so a perturbation delta per sample moves ln sigma and theta by at most delta sqrt(n) /
    (0.05 sqrt(n)) = 20 delta = 8e-9.  The bound asserted is 1e-7 (relative for the widths, radians
    for the angle): 250 delta, a factor 12 over that estimate for the columns' correlation and
    the minimiser's own stopping tolerance (1e-12)."""
    N = 128
    image_size = 0.05
    pixel = image_size / N
    major, minor, pa = 9 * pixel, 5 * pixel, math.radians(30.0)
    G = uv_taper_host((N, N), image_size, UVTaperParameters((major, minor, pa)))
    a = K * (5.0 / N) ** 2
    delta = (math.pi / a) * math.exp(-a * 64 ** 2) / (math.pi / (K * 45.0 / N ** 2))
    assert delta < 4e-10
    psf = np.fft.fftshift(np.fft.ifft2(np.fft.ifftshift(G)))
    # (row 0 and column 0 of G have no mirror image: part of the truncation, far below delta)
    assert np.abs(psf.imag).max() < delta * psf.real[N // 2, N // 2]
    psf = psf.real / psf.real[N // 2, N // 2]
    patch = psf[N // 2 - 20:N // 2 + 21, N // 2 - 20:N // 2 + 21]
    fitted = beam.fit_beam(patch, step=pixel)
    tol = 250 * 4e-10
    assert abs(fitted.major / major - 1) <= tol, fitted
    assert abs(fitted.minor / minor - 1) <= tol, fitted
    assert abs(fitted.theta - pa) <= tol, fitted
