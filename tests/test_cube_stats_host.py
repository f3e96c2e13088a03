"""Cube plane statistics on the host: the numpy twin (cube_stats.cube_stats_host) against an
independent statement of the contract on every case of cube_stats_cases -- per group np.sort of the
finite samples, the two middle elements, np.float32 arithmetic -- by bits wherever the statement has
no zero of either sign where np.sort's order of -0 and +0 could show, by ``==`` where it has; the
parameters' validation; update_noise's rules; and the noise the operator records, accepted by
MomentParameters(clip_sigma=...) on a cube whose smoothed planes cube smoothing's rule left NaN."""
import numpy as np
import pytest

import cube_stats_cases as cases
from katsdpimager_amd import cube_stats
from katsdpimager_amd.cube_stats import CubeStatsParameters


def test_keys_are_monotone_and_invertible():
    words = np.array([0xff7fffff, 0xbf800000, 0x80800000, 0x807fffff, 0x80000001, 0x80000000,
                      0x00000000, 0x00000001, 0x007fffff, 0x00800000, 0x3f800000, 0x7f7fffff], np.uint32)
    values = words.view(np.float32)
    keys = cube_stats.keys(values)
    assert keys.dtype == np.uint32 and (np.diff(keys.astype(np.int64)) > 0).all()
    assert keys[5] + 1 == keys[6]                       # -0 just below +0
    assert np.array_equal(cube_stats.values_of(keys).view(np.uint32), words)
    rng = np.random.default_rng(1)
    more = rng.integers(0, 2 ** 32, 5000, dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(cube_stats.values_of(cube_stats.keys(more.view(np.float32))).view(np.uint32), more)
    finite = more.view(np.float32)[np.isfinite(more.view(np.float32))]
    order = np.argsort(cube_stats.keys(finite), kind='stable')
    assert (np.diff(finite[order].astype(np.float64)) >= 0).all()


def test_twin_against_the_independent_statement():
    seen, groups, by_equality = set(), 0, 0
    for name, cube, filled, keywords, region in cases.host_cases():
        params = CubeStatsParameters(**keywords)
        got = cube_stats.cube_stats_host(cube, filled, params, region)
        first, stop = params.range(cube.shape[0])
        want, exact = cases.independent(cube, filled, first, stop, params.estimator, params.border,
                                        params.pool_polarizations, region)
        G = 1 if params.pool_polarizations else cube.shape[1]
        assert got.count.dtype == np.uint32 and got.count.shape == (cube.shape[0], G), name
        assert np.array_equal(got.count, want['count']), name
        for field in cases.FIELDS[1:]:
            a, b = getattr(got, field), want[field]
            assert a.dtype == np.float32 and a.shape == b.shape, (name, field)
            e = exact[field]
            assert np.array_equal(cases.bits(a)[e], cases.bits(b)[e]), (name, field)
            some = got.count > 0
            assert (a[~e & some] == b[~e & some]).all(), (name, field)
            by_equality += int((~e & some).sum())
            # no sample: 0x7fc00000, whatever the reason
            assert (cases.bits(a)[~some] == cases.QUIET_NAN).all(), (name, field)
        skipped = np.ones(cube.shape[0], bool)
        skipped[first:stop] = filled[first:stop] == 0
        assert (got.count[skipped] == 0).all(), name
        seen.add(name[0])
        groups += int((got.count > 0).sum())
        seen.update(int(n) for n in np.unique(got.count) if n <= 3)
    assert seen >= {'plane', 'mode', 'values', 'range', 'samples', 'one pixel', 0, 1, 2, 3}
    assert groups > 400 and by_equality > 10


def test_estimators_on_an_offset():
    """'median_abs' takes the offset for noise, 'mad' does not."""
    cube, filled, _ = cases.make_case(3, (1, 33, 65), 5, 'offset', sprinkle=False)
    plain = cube_stats.cube_stats_host(cube, filled, CubeStatsParameters())
    mad = cube_stats.cube_stats_host(cube, filled, CubeStatsParameters(estimator='mad'))
    on = filled != 0
    assert (plain.sigma[on] > 140).all() and (np.abs(mad.sigma[on] - 1.0) < 0.15).all()
    assert np.array_equal(plain.median, mad.median, equal_nan=True)
    assert (np.abs(np.abs(plain.median[on]) - 100.0) < 0.2).all()


def test_the_cube_is_not_written_and_inputs_are_checked():
    cube, filled, region = cases.make_case(3, (2, 7, 9), 3, region='sparse')
    before = cube.copy()
    cube_stats.cube_stats_host(cube, filled, CubeStatsParameters(estimator='mad'), region)
    assert np.array_equal(cases.bits(cube), cases.bits(before))
    params = CubeStatsParameters()
    with pytest.raises(TypeError):
        cube_stats.cube_stats_host(np.zeros(cube.shape, np.float64), filled, params)
    with pytest.raises(TypeError):
        cube_stats.cube_stats_host(cube, filled, dict())
    with pytest.raises(ValueError):
        cube_stats.cube_stats_host(cube[0], filled, params)
    with pytest.raises(ValueError):
        cube_stats.cube_stats_host(cube, filled[:2], params)
    with pytest.raises(ValueError):
        cube_stats.cube_stats_host(cube, filled, params, region[:, :8])
    with pytest.raises(TypeError):
        cube_stats.cube_stats_host(cube, filled, params, region.astype(np.int32))
    with pytest.raises(ValueError, match='border'):
        cube_stats.cube_stats_host(cube, filled, CubeStatsParameters(border=4))
    with pytest.raises(ValueError, match='beyond'):
        cube_stats.cube_stats_host(cube, filled, CubeStatsParameters(channels=(0, 4)))
    # a bool region is a region
    same = cube_stats.cube_stats_host(cube, filled, params, region != 0)
    cases.assert_same(same, cube_stats.cube_stats_host(cube, filled, params, region))


def test_parameter_validation():
    p = CubeStatsParameters()
    assert (p.estimator, p.border, p.pool_polarizations, p.channels) == ('median_abs', 0, True, None)
    assert p.range(7) == (0, 7) and p.groups(4) == 1
    q = CubeStatsParameters('mad', np.int64(3), False, (np.int32(2), 5))
    assert (q.estimator, q.border, q.pool_polarizations, q.channels) == ('mad', 3, False, (2, 5))
    assert q.range(5) == (2, 5) and q.groups(4) == 4 and type(q.border) is int
    assert 'mad' in repr(q) and '(2, 5)' in repr(q)
    assert CubeStatsParameters(border=2.0).border == 2
    for bad in ('mean', 'MAD', None, 0, b'mad'):
        with pytest.raises(ValueError, match='estimator'):
            CubeStatsParameters(estimator=bad)
    for bad in (-1, 1.5, True, False, np.True_, None, 'a', float('nan'), float('inf'), 2 ** 31):
        with pytest.raises(ValueError, match='border'):
            CubeStatsParameters(border=bad)
    for bad in (1, 0, None, 'yes'):
        with pytest.raises(ValueError, match='pool_polarizations'):
            CubeStatsParameters(pool_polarizations=bad)
    for bad in (3, (1,), (1, 2, 3), 'ab', (2, 2), (3, 2), (-1, 2), (0, 4097), (0.5, 2), (True, 2),
                (0, True), (None, 2)):
        with pytest.raises(ValueError):
            CubeStatsParameters(channels=bad)
    with pytest.raises(ValueError, match='beyond'):
        q.range(4)
    with pytest.raises(ValueError):
        p.range(0)
    with pytest.raises(ValueError):
        p.range(4097)
    with pytest.raises(ValueError, match='border'):
        q.check_plane(6, 9)
    q.check_plane(7, 9)


class _Cube:
    """What record_noise reads of a SpectralCube."""

    def __init__(self, filled, noise):
        self.filled = np.array(filled, np.uint8)
        self.noise = np.array(noise, np.float32)
        self.shape = (len(self.filled), 1, 1, 1)


def test_update_noise_rules():
    cube, filled, _ = cases.make_case(6, (2, 7, 9), 8, sprinkle=False)
    filled[:] = (1, 1, 0, 1, 1, 1)
    held = _Cube(filled, [9.0, np.nan, 7.0, np.nan, 5.0, np.nan])
    params = CubeStatsParameters(channels=(1, 5))
    result = cube_stats.cube_stats_host(cube, filled, params)
    cube_stats.record_noise(held, result, params)
    # channel 0 and 5: outside the range; channel 2: not filled; the others: measured
    assert held.noise[0] == 9.0 and np.isnan(held.noise[5]) and held.noise[2] == 7.0
    assert np.array_equal(held.noise[[1, 3, 4]], result.sigma[[1, 3, 4], 0])
    assert np.isfinite(held.noise[[1, 3, 4]]).all() and held.noise.dtype == np.float32
    per_plane = CubeStatsParameters(pool_polarizations=False)
    with pytest.raises(ValueError, match='pool_polarizations'):
        cube_stats.record_noise(held, cube_stats.cube_stats_host(cube, filled, per_plane), per_plane)


def test_recorded_noise_serves_clip_sigma_after_smoothing():
    """cube smoothing's rule leaves NaN for the planes it smoothed, and cut_table refuses them; with the
    measured noise recorded it makes the cuts."""
    from katsdpimager_amd import cube, smooth
    from katsdpimager_amd.beam import Beam
    rng = np.random.default_rng(4)
    C, P, H, W = 5, 1, 24, 28
    frequencies = 1.4e9 * (1.0 + 0.05 * np.arange(C) / (C - 1))
    beams = [Beam(1.0, 2.4 * frequencies[0] / f, 1.8 * frequencies[0] / f, 0.6) for f in frequencies]
    filled = np.array([1, 1, 0, 1, 1], np.uint8)
    beams[2] = None
    data = rng.normal(0.0, 1.0, (C, P, H, W)).astype(np.float32)
    noise = np.where(filled != 0, 1.0, np.nan).astype(np.float32)
    target = smooth.common_beam(beams, filled)
    radius, taps = smooth.kernel_tables(beams, target, filled)
    factors = smooth.flux_factors(beams, target, filled)
    smoothed = smooth.cube_smooth_host(data, filled, radius, taps)
    # CubeSmooth's rule for the returned cube's noise
    after = np.where((filled != 0) & (radius == 0), noise * factors, np.nan).astype(np.float32)
    assert np.isfinite(after[0]) and np.isnan(after[[1, 3, 4]]).all()
    moments = cube.MomentParameters((0,), axis='frequency', clip_sigma=3)
    with pytest.raises(ValueError, match='no noise recorded'):
        moments.cut_table(C, after, filled)
    held = _Cube(filled, after)
    params = CubeStatsParameters()
    result = cube_stats.cube_stats_host(smoothed, filled, params)
    cube_stats.record_noise(held, result, params)
    cut = moments.cut_table(C, held.noise, filled)
    on = filled != 0
    assert np.array_equal(cut[on], np.float32(3) * result.sigma[on, 0]) and np.isnan(cut[2])
    # white noise under the two widest kernels: clearly below the stand-in (the unsmoothed noise
    # times the factor)
    stand_in = noise * factors
    assert (held.noise[[3, 4]] < 0.8 * stand_in[[3, 4]]).all() and (held.noise[on] > 0.3).all()
