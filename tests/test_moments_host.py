"""Moment maps without a device: the numpy twin (cube.moments_host, the executable form of the
contract in include/kimg.h, "Moment maps") against truths that do not share its code -- the contract
restated per voxel in Python floats (moments_cases.restate), a Gaussian line whose moments are known
in closed form, and hand-made spectra -- then the cut and select_hanning, the parameters' refusals,
the velocity axis, the header's constants, the ABI surface and the argument checks of kimg_moments
(they run before any HIP call)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import moments_cases as cases
from katsdpimager_amd import cube

ALL = (0, 1, 2, 8, 9)


def _host(data, x, cut=None, filled=None, **keywords):
    """moments_host of spectra [C] or [C][...] with the cut of the parameters."""
    data = np.asarray(data, np.float32)
    if data.ndim == 1:
        data = data[:, None]
    C = data.shape[0]
    width = keywords.pop('channel_width', None)
    params = cube.MomentParameters(keywords.pop('moments', ALL), **keywords)
    if cut is None:
        cut = params.cut_table(C)
    elif np.ndim(cut) == 0:
        cut = np.full(C, cut, np.float32)
    filled = np.ones(C, np.uint8) if filled is None else filled
    return cube.moments_host(data, np.asarray(x, np.float64), cut, filled, params, channel_width=width)


# ---- the twin against the contract restated per voxel ----------------------------------------------
@pytest.mark.parametrize('C,plane,channels', [(1, (3,), None), (2, (7,), None), (3, (2, 5), None),
                                              (9, (4, 11), None), (9, (4, 11), (2, 7)),
                                              (33, (37,), (1, 32))])
@pytest.mark.parametrize('hanning', [False, True])
def test_twin_against_the_restatement(C, plane, channels, hanning):
    data, x, filled, cut = cases.random_cube(C, plane, 100 * C + len(plane) + hanning)
    params = cube.MomentParameters(ALL, channels=channels, select_hanning=hanning)
    first, stop = params.range(C)
    got = cube.moments_host(data, x, cut, filled, params, channel_width=2.5)
    width = cube.range_width(x, first, stop, 2.5)
    want = cases.restate(data, x, cut, filled, first, stop, hanning, width)
    assert set(got) == set(ALL) | {'count'}
    for key in want:
        cases.assert_same_bits(got[key], want[key], (key, C, plane, channels, hanning))
    if C >= 9:
        # the cases are not trivial: something entered, something did not, a peak was tied
        n = got['count']
        assert 0 < n.min() + 1 and n.max() > 1 and (n == 0).sum() < n.size
        flat = np.where(np.isfinite(data), data, -np.inf).reshape(C, -1)[first:stop]
        assert ((flat == flat.max(axis=0)).sum(axis=0) > 1).any()


@pytest.mark.parametrize('C', cases.SEAM_CHANNELS)
def test_twin_against_the_restatement_at_the_mask_seams(C):
    """The cases of test_moments_gpu.test_device_against_twin_at_the_mask_seams on a plane small
    enough for the loops: ranges that start and stop on and next to the seams of the device's `filled`
    bit mask, unfilled channels there, peaks in the range's end channels."""
    data, x, cut = cases.seam_cube(C, (2, 5, 6), 300 + C)
    for case in cases.seam_cases(C):
        first, stop, unfilled, hanning = case
        filled = cases.seam_filled(C, unfilled)
        params = cube.MomentParameters(ALL, channels=(first, stop), select_hanning=hanning)
        got = cube.moments_host(data, x, cut, filled, params, channel_width=2.5)
        width = cube.range_width(x, first, stop, 2.5)
        want = cases.restate(data, x, cut, filled, first, stop, hanning, width)
        for key in want:
            cases.assert_same_bits(got[key], want[key], (key, C) + case)
        cases.assert_seam_peaks(C, case, got[9], x)
        if stop - first > 2:
            assert got['count'].max() > 1 and (got['count'] < stop - first - len(unfilled) + 2).any()


def test_twin_against_the_restatement_at_the_longest_band():
    data, x, cut = cases.limit_cube(4096)
    C = cases.LIMIT_CHANNELS
    assert C == cube.MAX_CHANNELS
    for first, stop, unfilled, hanning in cases.limit_cases():
        filled = cases.seam_filled(C, unfilled)
        params = cube.MomentParameters(ALL, channels=(first, stop), select_hanning=hanning)
        got = cube.moments_host(data, x, cut, filled, params)
        want = cases.restate(data, x, cut, filled, first, stop, hanning, cube.range_width(x, first, stop))
        for key in want:
            cases.assert_same_bits(got[key], want[key], (key, first, stop, hanning))
        flat = got[9].reshape(-1)
        assert C - 1 in unfilled or flat[0] == np.float32(x[C - 1])
        assert flat[1] == np.float32(x[C - 2])


def test_restatement_width():
    x = np.array([10.0, 7.0, 5.0, 1.0])
    assert cube.range_width(x, 0, 4) == 3.0 and cube.range_width(x, 1, 3) == 2.0
    assert cube.range_width(x, 2, 3, -0.5) == 0.5
    with pytest.raises(ValueError):
        cube.range_width(x, 2, 3)


# ---- a Gaussian line ---------------------------------------------------------------------------------
def test_gaussian_line():
    """A Gaussian of area A, centre x0 and dispersion sigma sampled on 64 channels of spacing h.  The
    sums are the trapezoidal rule on a smooth function, whose error for a Gaussian (Euler-Maclaurin /
    Poisson summation) is 2 exp(-2 pi^2 sigma^2 / h^2) relative -- 1e-77 at sigma = 3 h -- plus the
    tails cut off at k sigma (k = 9.8 here: erfc(k / sqrt 2) and k phi(k) are below 1e-20).  What is
    left is rounding: each float32 sample carries a relative error of u = 2^-24, so
      moment 0: relative error <= u (samples) + u (output),
      moment 1: |error| <= u sum|I d| / S0 * 2 (numerator and denominator) + u |m1| (output),
      variance: |error| <= u (sum I d^2 / S0 * 2 + 2 |r| * 2 sum|I d| / S0), moment 2 = sqrt(variance):
                |error| <= that / (2 m2) + u m2,
    all evaluated below from the samples; float64 accumulation (2^-53 a step) is far below them."""
    C, h, sigma_ch = 64, 2.5, 3.0
    x = 400.0 - h * np.arange(C)                      # descending, as a frequency-ordered cube has it
    x0 = x[0] - 30.37 * h
    sigma = sigma_ch * h
    area = 7.5
    k = min(x[0] - x0, x0 - x[-1]) / sigma
    assert k >= 5 and math.erfc(k / math.sqrt(2)) < 1e-20
    assert 2 * math.exp(-2 * math.pi ** 2 * sigma_ch ** 2) < 1e-70
    exact = area / (sigma * math.sqrt(2 * math.pi)) * np.exp(-0.5 * ((x - x0) / sigma) ** 2)
    data = exact.astype(np.float32)
    out = _host(data, x, moments=(0, 1, 2))
    u = 2.0 ** -24
    d = x - x[C // 2]
    S0 = exact.sum()
    first_abs = np.abs(exact * d).sum() / S0
    second = (exact * d * d).sum() / S0
    r = abs(x0 - x[C // 2])
    assert abs(out[0][0] - area) <= area * 2 * u + 1e-15
    assert abs(out[1][0] - x0) <= 2 * u * first_abs + u * abs(x0) + 1e-12
    bound_var = u * (2 * second + 4 * r * first_abs)
    assert abs(out[2][0] - sigma) <= bound_var / (2 * sigma) + u * sigma + 1e-12
    assert out['count'][0] == C
    # (the bounds bind: they are a few float32 ulps, not a loose tolerance)
    assert 2 * u * first_abs + u * abs(x0) < 1e-4 and bound_var / (2 * sigma) + u * sigma < 1e-4


# ---- hand-made cases ---------------------------------------------------------------------------------
def test_constant_spectrum():
    n, h = 12, 1.5
    x = 100.0 + h * np.arange(n)
    out = _host(np.full(n, 0.25), x)
    assert out[0][0] == np.float32(0.25 * n * h)
    assert out[1][0] == np.float32(x.mean())
    assert abs(out[2][0] - h * math.sqrt((n * n - 1) / 12.0)) <= 2.0 ** -23 * out[2][0]
    assert out[8][0] == np.float32(0.25) and out[9][0] == np.float32(x[0]) and out['count'][0] == n


def test_single_entering_channel():
    x = 3.0 * np.arange(8) + 1.0
    data = np.zeros(8)
    data[5] = 2.0
    out = _host(data, x, cut=1.0)
    assert out['count'][0] == 1
    assert out[0][0] == np.float32(2.0 * 3.0) and out[1][0] == np.float32(x[5])
    assert out[2][0] == 0.0 and not np.signbit(out[2][0])
    assert out[8][0] == 2.0 and out[9][0] == np.float32(x[5])
    # a range of one channel takes its width from the caller
    one = _host(data, x, channels=(5, 6), channel_width=-3.0)
    assert one[0][0] == np.float32(6.0) and one[2][0] == 0.0
    with pytest.raises(ValueError):
        _host(data, x, channels=(5, 6))


def test_nothing_enters():
    x = np.arange(6.0)
    for data, cut, filled in ((np.ones(6), 5.0, None), (np.full(6, np.nan), None, None),
                              (np.ones(6), None, np.zeros(6, np.uint8)), (np.ones(6), np.nan, None)):
        out = _host(data, x, cut=cut, filled=filled)
        assert out['count'][0] == 0 and out['count'].dtype == np.int32
        assert all(np.isnan(out[m][0]) and out[m].dtype == np.float32 for m in ALL)


def test_sum_not_positive():
    x = np.arange(4.0)
    for data in ([1.0, -2.0, 0.5, 0.25], [1.0, -1.0, 0.5, -0.5]):
        out = _host(data, x)
        assert out['count'][0] == 4
        assert np.isnan(out[1][0]) and np.isnan(out[2][0])
        assert np.isfinite(out[0][0]) and out[8][0] == 1.0 and out[9][0] == 0.0
    assert _host([1.0, -1.0, 0.5, -0.5], x)[0][0] == 0.0


def test_tie_takes_the_first_channel():
    x = np.array([9.0, 7.0, 5.0, 3.0, 1.0])
    out = _host([1.0, 4.0, 2.0, 4.0, 4.0], x)
    assert out[8][0] == 4.0 and out[9][0] == 7.0
    out = _host([1.0, 4.0, 2.0, 4.0, 4.0], x, filled=np.array([1, 0, 1, 1, 1], np.uint8))
    assert out[9][0] == 3.0


# ---- the cut and select_hanning ----------------------------------------------------------------------
def test_cut_is_strict():
    x = np.arange(5.0)
    data = np.array([0.5, 1.25, 1.2500001, 3.0, -1.0], np.float32)
    out = _host(data, x, cut=1.25)
    assert out['count'][0] == 2 and out[9][0] == 3.0
    assert _host(data, x, cut=float(np.nextafter(np.float32(1.25), np.float32(0))))['count'][0] == 3
    # clip_sigma: float32(clip_sigma) * noise as a float32 product, per channel
    params = cube.MomentParameters(clip_sigma=3.0)
    noise = np.array([0.1, 0.2, np.nan, 0.4], np.float32)
    table = params.cut_table(4, noise, filled=np.array([1, 1, 0, 1]))
    assert table.dtype == np.float32
    assert np.array_equal(table[[0, 1, 3]], (np.float32(3.0) * noise)[[0, 1, 3]])
    with pytest.raises(ValueError):
        params.cut_table(4, noise, filled=np.ones(4))
    with pytest.raises(ValueError):
        params.cut_table(4)
    assert np.all(cube.MomentParameters().cut_table(3) == -np.inf)
    assert np.all(cube.MomentParameters(cut=0.5).cut_table(3) == np.float32(0.5))


def test_hanning_rejects_a_lone_spike():
    """Noise 1: a lone 3.9 sigma spike between neighbours at 0 smooths to 1.95 and misses the cut at
    3 sigma that the plain selection passes; a line three channels wide keeps its centre."""
    x = np.arange(9.0)
    spike = np.zeros(9)
    spike[4] = 3.9
    assert _host(spike, x, cut=3.0)['count'][0] == 1
    assert _host(spike, x, cut=3.0, select_hanning=True)['count'][0] == 0
    line = np.zeros(9)
    line[3:6] = 3.9
    out = _host(line, x, cut=3.0, select_hanning=True)
    assert out['count'][0] == 1 and out[9][0] == 4.0          # (0.25 + 0.5 + 0.25) * 3.9; the ends get 2.925
    # the sums take the samples themselves, not the smoothed ones
    assert out[0][0] == np.float32(3.9) * np.float32(1.0)


def test_hanning_replicates_at_edges_and_gaps():
    x = np.arange(6.0)
    # at the range's edge the missing neighbour is the sample itself: 0.75 * 3.9 + 0.25 * 0 = 2.925
    edge = np.array([3.9, 0, 0, 0, 0, 0])
    assert _host(edge, x, cut=2.9, select_hanning=True)['count'][0] == 1
    assert _host(edge, x, cut=2.93, select_hanning=True)['count'][0] == 0
    # the range, not the band, makes the edge
    inner = np.array([0, 0, 3.9, 0, 0, 0])
    assert _host(inner, x, cut=2.9, select_hanning=True)['count'][0] == 0
    assert _host(inner, x, cut=2.9, select_hanning=True, channels=(2, 6))['count'][0] == 1
    # next to a NaN, and next to a channel that is not filled, likewise
    gap = np.array([0, np.nan, 3.9, 0, 0, 0])
    assert _host(gap, x, cut=2.9, select_hanning=True)['count'][0] == 1
    hole = np.array([0, 7.0, 3.9, 0, 0, 0])
    filled = np.array([1, 0, 1, 1, 1, 1], np.uint8)
    assert _host(hole, x, cut=2.9, select_hanning=True, filled=filled)['count'][0] == 1
    # between two gaps the sample stands alone: s = I
    alone = np.array([np.nan, 3.9, np.inf, 0, 0, 0])
    out = _host(alone, x, cut=3.8, select_hanning=True)
    assert out['count'][0] == 1 and out[8][0] == np.float32(3.9)


# ---- parameters, coordinates, header -----------------------------------------------------------------
def test_parameters():
    p = cube.MomentParameters()
    assert p.moments == (0, 1, 2) and p.axis == 'velocity' and not p.select_hanning
    assert p.range(7) == (0, 7)
    p = cube.MomentParameters([9, 0], 'frequency', channels=(2, 5), clip_sigma=3, select_hanning=True)
    assert p.moments == (0, 9) and p.range(5) == (2, 5)
    assert repr(p) == "MomentParameters((0, 9), axis='frequency', channels=(2, 5), clip_sigma=3.0, " \
                      "select_hanning=True)"
    assert 'rest_frequency=1420405751.77' in repr(cube.MomentParameters(rest_frequency=1420405751.77))
    with pytest.raises(ValueError):
        p.range(4)
    for bad in (dict(moments=()), dict(moments=(3,)), dict(moments=(0, 0)), dict(moments=(1.0,)),
                dict(moments=(True,)), dict(moments=5), dict(axis='optical'),
                dict(rest_frequency=0.0), dict(rest_frequency=float('nan')),
                dict(rest_frequency=float('inf')), dict(channels=(3, 3)), dict(channels=(-1, 2)),
                dict(channels=(0, 1.5)), dict(channels=(0, 4097)), dict(channels=5),
                dict(channels=(0, float('nan'))), dict(clip_sigma=3, cut=0.1),
                dict(clip_sigma=float('nan')), dict(cut=float('nan')), dict(cut='x'),
                dict(select_hanning=1)):
        with pytest.raises(ValueError):
            cube.MomentParameters(**bad)
    with pytest.raises(ValueError):
        cube.MomentParameters().range(4097)
    assert cube.moment_bunit(0) == 'Jy/beam.km/s' and cube.moment_bunit(8, 'K') == 'K'
    assert [cube.moment_bunit(m) for m in (1, 2, 9)] == ['km/s'] * 3
    assert cube.moment_bunit(0, axis='frequency') == 'Jy/beam.Hz'


def test_velocity_axis():
    f0 = 1420405751.77
    frequencies = f0 + 1.0e5 * np.arange(-3, 4) + 1234.5
    got = cube.velocities(frequencies, f0)
    assert got.dtype == np.float64
    assert got.tolist() == [(1.0 - float(f) / f0) * 299792.458 for f in frequencies]
    assert got[0] > 0 > got[-1]                         # a lower frequency recedes
    with pytest.raises(ValueError):
        cube.velocities(frequencies, 0.0)


def test_twin_refusals():
    p = cube.MomentParameters()
    x, cut, filled = np.arange(3.0), np.zeros(3, np.float32), np.ones(3)
    with pytest.raises(TypeError):
        cube.moments_host(np.zeros((3, 2)), x, cut, filled, p)
    with pytest.raises(ValueError):
        cube.moments_host(np.zeros(3, np.float32), x, cut, filled, p)
    with pytest.raises(ValueError):
        cube.moments_host(np.zeros((3, 2), np.float32), x[:2], cut, filled, p)
    with pytest.raises(ValueError):
        cube.moments_host(np.zeros((3, 2), np.float32), x, cut, filled[:2], p)


def test_symbol_is_declared_exported_and_prototyped():
    from katsdpimager_amd import _lib, build
    assert 'moments.hip' in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, 'moments.hip'))
    assert 'kimg_moments' in _lib.PROTOTYPES
    assert _lib.lib().kimg_moments is not None
    header = open(os.path.join(os.path.dirname(build.HERE), 'include', 'kimg.h')).read()
    assert re.search(r'^int kimg_moments\(', header, re.M)
    defines = dict(re.findall(r'^#define (KIMG_MOMENTS?_\w+) (\d+)$', header, re.M))
    assert int(defines['KIMG_MOMENTS_MAX_CHANNELS']) == cube.MAX_CHANNELS == 4096
    for key, name in ((0, '0'), (1, '1'), (2, '2'), (8, '8'), (9, '9'), ('count', 'COUNT')):
        assert int(defines['KIMG_MOMENT_' + name]) == cube.MOMENT_BITS[key]
    assert len(defines) == 7
    source = open(os.path.join(build.CSRC, 'moments.hip')).read()
    assert 'MM_MAX_CHANNELS = KIMG_MOMENTS_MAX_CHANNELS;' in source
    assert _lib.lib().kimg_version() == _lib.VERSION == 5


def test_argument_errors_come_before_any_launch():
    from katsdpimager_amd import _lib
    memory = np.zeros(4096 + 4, np.float64)
    pointer = memory.ctypes.data + (-memory.ctypes.data % 16)
    assert cases.abi_errors(_lib.lib(), pointer) == 21
    assert not memory.any()
