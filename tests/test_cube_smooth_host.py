"""Cube smoothing to a common beam without a device: the host code that chooses the common beam and
makes the taps (smooth.common_beam, smooth.kernel_tables), the numpy twin of the convolution
(smooth.cube_smooth_host) against a float64 direct convolution, against the exact Gaussian it must
produce and against the contract's exact semantics on hand-made planes, and the argument checks of
kimg_cube_smooth (they run before any HIP call)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import cube_smooth_cases as cases
from katsdpimager_amd import smooth
from katsdpimager_amd.beam import Beam


def _random_beams(rng, n):
    return [Beam(1.0, rng.uniform(1.0, 4.0), rng.uniform(1.0, 4.0), rng.uniform(0.0, math.pi))
            for _ in range(n)]


def _same(a, b):
    return (a.model.x_stddev.value, a.model.y_stddev.value, float(a.model.theta)) \
        == (b.model.x_stddev.value, b.model.y_stddev.value, float(b.model.theta))


def test_common_beam_contains_every_beam():
    rng = np.random.default_rng(1)
    for trial in range(20):
        beams = _random_beams(rng, 1 + trial % 7)
        target = smooth.common_beam(beams)
        sigma_t = smooth.beam_covariance(target)
        areas = [math.sqrt(np.linalg.det(smooth.beam_covariance(b))) for b in beams]
        largest = smooth.beam_covariance(beams[int(np.argmax(areas))])
        # a scaled copy of the largest beam ...
        s = sigma_t[0, 0] / largest[0, 0]
        assert s >= 1.0 - 1e-12 and np.allclose(sigma_t, s * largest, rtol=1e-12, atol=0.0)
        lowest = []
        for b in beams:
            value = np.linalg.eigvalsh(sigma_t - smooth.beam_covariance(b))
            assert value[0] >= -1e-9 * np.trace(sigma_t)
            lowest.append(value[0] / np.trace(sigma_t))
        # ... and the smallest: some beam touches it (or it is the largest beam itself)
        assert min(lowest) <= 1e-9
        smooth.kernel_tables(beams, target, truncate=1.0)        # (no refusal)


def test_common_beam_of_frequency_scaled_copies_is_the_largest():
    frequencies = 1.4e9 * (1.0 + 0.05 * np.arange(8) / 7.0)
    for theta in (0.0, 0.3, 2.0):
        beams = [Beam(1.0, 2.7 * frequencies[0] / f, 1.9 * frequencies[0] / f, theta) for f in frequencies]
        assert _same(smooth.common_beam(beams), beams[0])
        assert _same(smooth.common_beam(beams[::-1]), beams[0])
        # unfilled channels do not count, with or without a beam
        filled = np.ones(8, np.uint8)
        filled[0] = 0
        assert _same(smooth.common_beam(beams, filled), beams[1])
        assert _same(smooth.common_beam([None] + beams[1:]), beams[1])
    # ties go to the lowest channel
    a, b = Beam(1.0, 3.0, 2.0, 0.0), Beam(1.0, 2.0, 3.0, 0.0)
    for pair in ((a, b), (b, a)):
        sigma = smooth.beam_covariance(smooth.common_beam(pair))
        assert np.allclose(sigma, 2.25 * smooth.beam_covariance(pair[0]), rtol=1e-12)
    with pytest.raises(ValueError):
        smooth.common_beam([])
    with pytest.raises(ValueError):
        smooth.common_beam([None, None])
    with pytest.raises(ValueError):
        smooth.common_beam([a, None], filled=[1, 1])


def test_common_beam_does_not_depend_on_the_order():
    rng = np.random.default_rng(2)
    for trial in range(10):
        beams = _random_beams(rng, 6)
        want = smooth.common_beam(beams)
        for _ in range(4):
            assert _same(smooth.common_beam([beams[i] for i in rng.permutation(6)]), want)


def test_taps_sum_to_the_flux_factor():
    rng = np.random.default_rng(3)
    seen = set()
    for trial in range(12):
        major, minor, theta = rng.uniform(2.0, 2.6), rng.uniform(1.6, 2.0), rng.uniform(0.0, math.pi)
        beams = [Beam(1.0, s * major, s * minor, theta) for s in (1.0, 0.9995, 0.97, 0.85)]
        target = smooth.common_beam(beams)
        for units in ('beam', 'pixel'):
            radius, taps = smooth.kernel_tables(beams, target, truncate=4.0, units=units)
            factors = smooth.flux_factors(beams, target, units=units)
            assert radius.dtype == np.int32 and taps.dtype == np.float32 and taps.shape == (4, 33 * 33)
            for c in range(4):
                R = int(radius[c])
                seen.add(R)
                count = (2 * R + 1) ** 2
                sigma_t, sigma_c = smooth.beam_covariance(target), smooth.beam_covariance(beams[c])
                want = math.sqrt(np.linalg.det(sigma_t) / np.linalg.det(sigma_c)) if units == 'beam' else 1.0
                assert abs(factors[c] - want) <= 1e-14 * want and 1.0 <= want < 2.0
                total = taps[c, :count].astype(np.float64).sum()
                assert abs(total - want) <= count * 2.0 ** -24
                assert not taps[c, count:].any()
                # symmetric about the centre, largest there
                grid = taps[c, :count].reshape(2 * R + 1, 2 * R + 1)
                assert np.array_equal(grid, grid[::-1, ::-1]) and grid.argmax() == count // 2
    assert 0 in seen and max(seen) >= 4


def _radius_of(sigma_k, truncate=4.0, minor=None):
    """Through the beams: a round beam of sigma 2 taken to the one whose kernel has ``sigma_k``."""
    source = Beam(1.0, 2.0, 2.0, 0.0)
    minor = sigma_k if minor is None else minor
    target = Beam(1.0, math.sqrt(4.0 + sigma_k ** 2), math.sqrt(4.0 + minor ** 2), 0.0)
    return int(smooth.kernel_tables([source], target, truncate=truncate)[0][0])


def test_radius_rule_at_its_thresholds():
    assert smooth.kernel_radius(0.049) == 0 and smooth.kernel_radius(0.05) == 1
    assert smooth.kernel_radius(0.0) == 0 and smooth.kernel_radius(0.05, truncate=6.0) == 1
    eps = 1e-6
    assert _radius_of(0.049) == 0 and _radius_of(0.05 - eps) == 0 and _radius_of(0.05 + eps) == 1
    for truncate in (4.0, 6.0, 2.5):
        for k in range(1, 17):
            if truncate == 4.0:                                 # (k / 4 is exact)
                assert smooth.kernel_radius(k / truncate, truncate) == k
            if k / truncate - eps >= 0.05:
                assert _radius_of(k / truncate - eps, truncate) == k
            if k < 16:
                assert _radius_of(k / truncate + eps, truncate) == k + 1
        with pytest.raises(ValueError, match='ConvolveBeam'):
            _radius_of(16.0 / truncate + eps, truncate)
    # the larger sigma decides, whichever axis it is on, and the smaller is floored at 1e-3 px
    assert _radius_of(1.0 + eps, minor=0.0) == 5 and _radius_of(0.0, minor=1.0 + eps) == 5
    radius, taps = smooth.kernel_tables([Beam(1.0, 2.0, 2.0, 0.0)], Beam(1.0, math.sqrt(4.81), 2.0, 0.0))
    grid = taps[0, :81].reshape(9, 9).astype(np.float64)
    assert radius[0] == 4 and not grid[:, :4].any() and not grid[:, 5:].any()
    profile = np.exp(-0.5 * (np.arange(-4, 5) / 0.9) ** 2.0)     # along axis 0, which is x of a Beam
    assert np.allclose(grid[:, 4], profile / profile.sum() * math.sqrt(4.81) / 2.0, rtol=1e-6)


def test_refusals():
    small, large = Beam(1.0, 2.0, 1.5, 0.4), Beam(1.0, 2.5, 2.0, 0.4)
    with pytest.raises(ValueError, match='channel 1'):
        smooth.kernel_tables([small, large], small)             # the target does not contain a beam
    with pytest.raises(ValueError, match='does not contain'):
        smooth.kernel_tables([Beam(1.0, 2.0, 1.5, 0.0)], Beam(1.0, 2.0, 1.5, 1.0))
    smooth.kernel_tables([small, large], small, filled=[1, 0])  # ... unless that channel is not filled
    with pytest.raises(ValueError, match='channel 1'):
        smooth.kernel_tables([small, None], large, filled=[1, 1])       # a missing beam
    assert smooth.kernel_tables([small, None], large)[0].tolist() \
        == smooth.kernel_tables([small, None], large, filled=[1, 0])[0].tolist()
    with pytest.raises(ValueError, match='channel 0.*ConvolveBeam'):
        smooth.kernel_tables([small], Beam(1.0, 5.0, 4.5, 0.4))  # R > 16
    assert smooth.kernel_tables([small], Beam(1.0, 5.0, 4.5, 0.4), truncate=3.0)[0][0] == 14
    # the flux factor depends neither on truncate nor on the radius: a kernel sigma above 4 px is
    # none of its business
    factor = smooth.flux_factors([small], Beam(1.0, 5.0, 4.5, 0.4))[0]
    assert abs(factor - 5.0 * 4.5 / (2.0 * 1.5)) <= 1e-13 * factor
    assert smooth.flux_factors([small], Beam(1.0, 50.0, 45.0, 0.4), units='pixel')[0] == 1.0
    with pytest.raises(ValueError, match='does not contain'):
        smooth.flux_factors([large], small)
    with pytest.raises(ValueError, match='channel 1'):
        smooth.flux_factors([small, None], large, filled=[1, 1])
    with pytest.raises(ValueError):
        smooth.kernel_tables([small], large, units='Jy')
    for bad in (0.0, -1.0, np.inf, np.nan, 'a'):
        with pytest.raises(ValueError):
            smooth.kernel_tables([small], large, truncate=bad)
        with pytest.raises(ValueError):
            smooth.CommonBeamParameters(truncate=bad)
    with pytest.raises(TypeError):
        smooth.kernel_tables([small], (2.5, 2.0, 0.4))
    with pytest.raises(TypeError):
        smooth.CommonBeamParameters(target=(2.5, 2.0, 0.4))
    with pytest.raises(ValueError):
        smooth.CommonBeamParameters(units='Jy')
    with pytest.raises(TypeError):
        smooth.CubeSmoothTemplate(None, object())
    # the twin's own
    cube = np.zeros((2, 1, 3, 3), np.float32)
    taps = np.zeros((2, 9), np.float32)
    with pytest.raises(TypeError):
        smooth.cube_smooth_host(cube.astype(np.float64), [1, 1], [0, 0], taps)
    with pytest.raises(TypeError):
        smooth.cube_smooth_host(cube, [1, 1], [0, 0], taps.astype(np.float64))
    with pytest.raises(ValueError):
        smooth.cube_smooth_host(cube[0], [1, 1], [0, 0], taps)
    with pytest.raises(ValueError):
        smooth.cube_smooth_host(cube, [1], [0, 0], taps)
    with pytest.raises(ValueError):
        smooth.cube_smooth_host(cube, [1, 1], [0, 17], taps)
    with pytest.raises(ValueError):
        smooth.cube_smooth_host(cube, [1, 1], [0, 2], taps)     # 25 taps in a table of 9
    smooth.cube_smooth_host(cube, [1, 0], [0, 17], taps)


@pytest.mark.parametrize('C', [1, 2, 5])
def test_twin_against_float64_convolution(C):
    checked = 0
    for i, plane in enumerate(((1, 1, 1), (1, 3, 5), (2, 7, 9), (1, 5, 65), (1, 40, 37))):
        cube, filled, radius, taps = cases.make_case(C, plane, 10 * C + i)
        held = cube.copy()
        got = smooth.cube_smooth_host(cube, filled, radius, taps)
        assert got.dtype == np.float32 and got.shape == cube.shape
        checked += cases.assert_within_bound(got, cube, filled, radius, taps, (C, plane))
        assert np.array_equal(cases.bits(cube), cases.bits(held))
        nan = np.isnan(got[filled != 0])
        assert (cases.bits(got[filled != 0])[nan] == cases.QUIET_NAN).all()
    assert checked > 1000


def _gaussian(sigma, shape):
    inverse = np.linalg.inv(sigma)
    y = np.arange(shape[0], dtype=np.float64)[:, None] - shape[0] // 2
    x = np.arange(shape[1], dtype=np.float64)[None, :] - shape[1] // 2
    return np.exp(-0.5 * (inverse[0, 0] * y * y + 2.0 * inverse[0, 1] * y * x + inverse[1, 1] * x * x))


@pytest.mark.parametrize('source,target', [
    ((1.5, 1.5, 0.0), (1.9, 1.9, 0.0)),
    ((2.0, 1.5, 0.5), (2.6, 2.1, 0.5)),
    ((2.2, 1.6, 0.3), (3.0, 2.5, 1.2)),
])
def test_point_source_becomes_the_target_gaussian(source, target):
    """A point source restored with beam c -- the exact Gaussian of Sigma_c, peak 1 -- smoothed to
    T with truncate = 6 is the exact Gaussian of Sigma_T, peak 1, in Jy/beam: the continuous
    convolution of the two Gaussians has the covariance Sigma_T and the peak sqrt(det Sigma_c /
    det Sigma_T), which the flux factor undoes.  What the sampled, truncated kernel adds, per pixel
    and for an input of at most 1: the mass of a 2-D Gaussian beyond t sigma, e^(-t^2/2), with the
    same again for renormalising the rest (1 + t^2/2 covers both for t >= 2); the aliasing of a
    Gaussian of sigma_min sampled at unit spacing, 2 e^(-2 pi^2 sigma_min^2) (its transform at the
    first image, both signs); and the float32 arithmetic, cube_smooth_cases.bound."""
    t = 6.0
    beam_c, beam_t = Beam(1.0, *source), Beam(1.0, *target)
    sigma_c, sigma_t = smooth.beam_covariance(beam_c), smooth.beam_covariance(beam_t)
    kernel = np.linalg.eigvalsh(sigma_t - sigma_c)
    sigma_min = math.sqrt(kernel[0])
    assert sigma_min >= 1.0 and min(source[:2]) >= 1.5
    shape = (81, 80)
    plane = _gaussian(sigma_c, shape).astype(np.float32)
    cube = plane[None, None]
    radius, taps = smooth.kernel_tables([beam_c], beam_t, truncate=t)
    R = int(radius[0])
    assert R == math.ceil(t * math.sqrt(kernel[1])) <= 16
    got = smooth.cube_smooth_host(cube, [1], radius, taps)[0, 0].astype(np.float64)
    _, S = cases.direct(cube[0], taps[0], R)
    limit = math.exp(-0.5 * t * t) * (1.0 + 0.5 * t * t) + 2.0 * math.exp(-2.0 * math.pi ** 2 * sigma_min ** 2) \
        + cases.bound(R, S[0])
    error = np.abs(got - _gaussian(sigma_t, shape))
    print('worst error', error.max(), 'bound there', limit.reshape(-1)[error.argmax()])
    assert (error <= limit).all()
    assert abs(got[shape[0] // 2, shape[1] // 2] - 1.0) <= limit[shape[0] // 2, shape[1] // 2]
    # Jy/pixel: the sum of the plane is kept -- every tap reaches every sample well inside the
    # border, so the sum is the sum of the taps (1 within (2R + 1)^2 2^-24) times the plane's, to the
    # float32 arithmetic of every pixel
    radius, taps = smooth.kernel_tables([beam_c], beam_t, truncate=t, units='pixel')
    got = smooth.cube_smooth_host(cube, [1], radius, taps)[0, 0].astype(np.float64)
    total = plane.astype(np.float64).sum()
    _, S = cases.direct(cube[0], taps[0], R)
    limit = cases.bound(R, S).sum() + (2 * R + 1) ** 2 * 2.0 ** -24 * total
    # (what leaves through the border: the plane is below e^-50 there)
    assert plane[:R + 1].max() < 1e-20 and plane[:, :R + 1].max() < 1e-20
    print('sum', got.sum(), 'of', total, 'bound', limit)
    assert abs(got.sum() - total) <= limit


def _ones_taps(R, value=1.0):
    taps = np.zeros((1, 33 * 33), np.float32)
    taps[0, :(2 * R + 1) ** 2] = value
    return taps


def test_nan_and_inf_spread_over_their_footprint():
    R = 2
    for payload in (0x7fc12345, 0xffc00001, 0x7fc00000, 0x7f800001):
        plane = np.ones((1, 1, 11, 12), np.float32)
        plane.view(np.uint32)[0, 0, 4, 7] = payload
        got = smooth.cube_smooth_host(plane, [1], [R], _ones_taps(R, 0.04))
        nan = np.zeros(plane.shape, bool)
        nan[0, 0, 2:7, 5:10] = True
        assert np.array_equal(np.isnan(got), nan)
        assert (cases.bits(got)[nan] == cases.QUIET_NAN).all()
        assert np.isfinite(got[~nan]).all()
    plane = np.ones((1, 1, 11, 12), np.float32)
    plane[0, 0, 4, 3] = np.inf
    plane[0, 0, 4, 6] = -np.inf
    got = smooth.cube_smooth_host(plane, [1], [R], _ones_taps(R, 0.04))[0, 0]
    assert (got[2:7, 1:4] == np.inf).all() and (got[2:7, 6:9] == -np.inf).all()
    assert (cases.bits(got[2:7, 4:6]) == cases.QUIET_NAN).all()         # inf - inf
    rest = np.ones(got.shape, bool)
    rest[2:7, 1:9] = False
    assert np.isfinite(got[rest]).all()
    # a negative tap turns the sign of an Inf
    taps = _ones_taps(1, 0.1)
    taps[0, 0] = -0.1                                                   # (dy, dx) = (-1, -1)
    plane = np.zeros((1, 1, 5, 5), np.float32)
    plane[0, 0, 2, 2] = np.inf
    got = smooth.cube_smooth_host(plane, [1], [1], taps)[0, 0]
    assert got[3, 3] == -np.inf and (np.delete(got[1:4, 1:4].reshape(-1), 8) == np.inf).all()


def test_zero_border_and_signed_zeros():
    """Beyond the plane a sample is +0.0, multiplied and added like any other.  The accumulator
    starts as +0.0 and +0.0 + (-0.0) = +0.0, so it is never -0.0: a plane of -0.0, whose every
    product is -0.0, comes out as +0.0, in a scaled copy (R = 0) too, and so does a corner pixel
    whose border products are -0.0 (negative taps over +0.0)."""
    plane = np.full((1, 1, 3, 4), -0.0, np.float32)
    for R in (0, 1, 3):
        got = smooth.cube_smooth_host(plane, [1], [R], _ones_taps(R, 0.5))
        assert (cases.bits(got) == 0).all()
        got = smooth.cube_smooth_host(-plane, [1], [R], _ones_taps(R, -0.5))
        assert (cases.bits(got) == 0).all()
    # sums next to the border: only the samples inside count
    plane = np.arange(1, 13, dtype=np.float32).reshape(1, 1, 3, 4)
    got = smooth.cube_smooth_host(plane, [1], [1], _ones_taps(1))[0, 0]
    assert got[0, 0] == 1 + 2 + 5 + 6 and got[2, 3] == 7 + 8 + 11 + 12 and got[1, 1] == 78 - 4 - 8 - 12
    # an infinite tap over the border makes a NaN there, as the contract's arithmetic says
    taps = _ones_taps(1)
    taps[0, 0] = np.inf
    got = smooth.cube_smooth_host(plane, [1], [1], taps)[0, 0]
    assert (cases.bits(got[0]) == cases.QUIET_NAN).all() and (cases.bits(got[:, 0]) == cases.QUIET_NAN).all()
    assert (got[1:, 1:] == np.inf).all()


def test_radius_larger_than_the_plane():
    R = 3
    taps = np.zeros((1, 33 * 33), np.float32)
    taps[0, :49] = np.linspace(0.1, 0.9, 49, dtype=np.float32)
    plane = np.full((1, 1, 1, 1), 3.0, np.float32)
    got = smooth.cube_smooth_host(plane, [1], [R], taps)
    assert got.shape == (1, 1, 1, 1) and got[0, 0, 0, 0] == taps[0, 24] * np.float32(3.0)
    cube, filled, radius, taps = cases.make_case(1, (2, 2, 3), 5, radii=[7])
    cases.assert_within_bound(smooth.cube_smooth_host(cube, filled, radius, taps), cube, filled, radius, taps)


def test_unfilled_channels_and_scaled_copies():
    cube, filled, radius, taps = cases.make_case(5, (2, 7, 9), 8, radii=[0, 2, 0, 1, 0])
    assert filled.tolist() == [1, 1, 1, 1, 0]
    sentinel = np.full(cube.shape, -3.0e38, np.float32)
    got = smooth.cube_smooth_host(cube, filled, radius, taps, out=sentinel)
    assert (got[4] == np.float32(-3.0e38)).all() and (sentinel == np.float32(-3.0e38)).all()
    assert np.isnan(smooth.cube_smooth_host(cube, filled, radius, taps)[4]).all()
    with np.errstate(all='ignore'):
        for c in (0, 2):
            want = np.float32(0.0) + taps[c, 0] * cube[c]
            want = np.where(np.isnan(want), np.array([cases.QUIET_NAN], np.uint32).view(np.float32)[0], want)
            assert np.array_equal(cases.bits(got[c]), cases.bits(want))
    # a channel's result is its own: it does not depend on the others
    alone = smooth.cube_smooth_host(cube[1:2], [1], radius[1:2], taps[1:2])
    assert np.array_equal(cases.bits(alone[0]), cases.bits(got[1]))


def test_argument_errors_return_their_codes():
    from katsdpimager_amd import _lib
    C, M = 8, 64
    memory = np.full(2 * C * M + 8, 7.0, np.float32)
    taps = np.ones(C * 33 * 33 + 4, np.float32)
    base = memory.ctypes.data
    base += -base % 16
    table = taps.ctypes.data
    table += -table % 16
    checked = cases.abi_errors(_lib.lib(), base, base + 4 * C * M, table)
    assert checked == 34
    assert (memory == 7.0).all() and (taps == 1.0).all()


def test_symbol_is_declared_exported_and_prototyped():
    from katsdpimager_amd import _lib, build, cube
    assert 'cube_smooth.hip' in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, 'cube_smooth.hip'))
    restype, argtypes = _lib.PROTOTYPES['kimg_cube_smooth']
    assert restype is ctypes.c_int and len(argtypes) == 13
    assert _lib.lib().kimg_cube_smooth is not None
    header = open(os.path.join(os.path.dirname(build.HERE), 'include', 'kimg.h')).read()
    declaration = re.search(r'^int kimg_cube_smooth\(([^;]*)\);', header, re.M).group(1)
    assert declaration.count(',') + 1 == 13
    assert 'Cube smoothing to a common beam' in header
    assert int(re.search(r'^#define KIMG_CUBE_SMOOTH_MAX_RADIUS (\d+)$', header, re.M).group(1)) \
        == smooth.MAX_RADIUS == 16
    assert smooth.TAPS_PITCH == 33 * 33 and smooth.MAX_CHANNELS == cube.MAX_CHANNELS
    assert '#include "kimg_cube_column.h"' in open(os.path.join(build.CSRC, 'cube_smooth.hip')).read()
