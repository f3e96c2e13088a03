"""The numpy twin of kimg_spectrum_stats (spectrum_stats.spectrum_stats_host) against the contract
restated per voxel in plain Python (spectrum_stats_cases.restate_voxel), by bits, and the
parameters' validation.  No GPU."""
import numpy as np
import pytest

import spectrum_stats_cases as cases
from katsdpimager_amd import spectrum_stats
from katsdpimager_amd.spectrum_stats import SpectrumStatsParameters, spectrum_stats_host


def _compare(cube, filled, keywords, where):
    params = SpectrumStatsParameters(**keywords)
    C = cube.shape[0]
    enter = params.entering(C, filled)
    maps, line = spectrum_stats_host(cube, filled, params, subtract=True)
    want, want_line = cases.restate(cube, enter, filled, params.estimator, params.min_samples, subtract=True)
    for name in cases.FIELDS:
        cases.assert_same_bits(maps[name], want[name], where + (name,))
    cases.assert_same_bits(line, want_line, where + ('line',))
    # channels that are not filled keep the input's bits
    off = np.asarray(filled) == 0
    assert np.array_equal(cases.bits(line[off]), cases.bits(cube[off]))
    alone = spectrum_stats_host(cube, filled, params)
    assert set(alone) == set(cases.FIELDS)
    return maps, enter


@pytest.mark.parametrize('values', cases.VALUE_SETS)
def test_twin_against_restatement_on_the_value_sets(values):
    for estimator in cases.ESTIMATORS:
        for C, plane in ((1, (1, 2, 3)), (2, (1, 2, 3)), (9, (2, 3, 4)), (40, (1, 3, 5))):
            cube = cases.value_cube(values, C, plane, 3 * C + len(values))
            filled = cases.seam_filled(C, C)
            maps, enter = _compare(cube, filled, dict(estimator=estimator), (values, estimator, C))
            if values not in ('non_finite',) and enter.any():
                assert maps['count'].max() == enter.sum()
    if values == 'every_exponent':
        cube = cases.value_cube(values, 510, (1, 1, 4), 5)
        maps, _ = _compare(cube, np.ones(510, np.uint8), dict(estimator='mad'), (values, 510))
        assert (maps['count'] == 510).all()
    if values == 'huge':
        cube = cases.value_cube(values, 8, (1, 8, 8), 1)
        maps, _ = _compare(cube, np.ones(8, np.uint8), dict(estimator='mad', outputs=('median', 'sigma')),
                           (values, 'overflow'))
        assert np.isinf(maps['median']).any() and np.isinf(maps['sigma']).any()
        assert not np.isnan(maps['sigma']).any()


def test_twin_against_restatement_on_counts_ranges_and_min_samples():
    C, plane = 12, (1, 4, 8)
    cube = cases.counts_cube(C, plane, 7)
    filled = np.ones(C, np.uint8)
    for min_samples in (1, 3, 6, C, C + 1):
        for estimator in cases.ESTIMATORS:
            maps, _ = _compare(cube, filled, dict(estimator=estimator, min_samples=min_samples),
                               ('counts', estimator, min_samples))
            n = maps['count'].reshape(-1)
            assert set(n[:8].tolist()) == {0, 1, 2, 3, 4, 5, C - 1, C}
            for name in cases.FIELDS[:4]:
                assert np.array_equal(np.isnan(maps[name]).reshape(-1), n < min_samples), (name, min_samples)
    # a range, exclusions, unfilled channels: n counts the entering channels only, the line covers
    # every filled one
    cube = cases.noise_cube(20, (2, 3, 5), 9, nan_fraction=0.0)
    cube[np.isinf(cube)] = 1.0
    filled = np.ones(20, np.uint8)
    filled[[3, 11, 19]] = 0
    keywords = dict(channels=(2, 17), exclude_ranges=[(5, 8), (10, 12)])
    maps, enter = _compare(cube, filled, keywords, ('range',))
    assert enter.tolist() == [c in (2, 4, 8, 9, 12, 13, 14, 15, 16) for c in range(20)]
    assert (maps['count'] == 9).all()
    _, line = spectrum_stats_host(cube, filled, SpectrumStatsParameters(**keywords), subtract=True)
    for c in (0, 1, 5, 18):         # filled, outside the range or excluded: subtracted all the same
        assert np.array_equal(cases.bits(line[c]), cases.bits(cube[c] - maps['median']))
    # S = 0: nothing enters, n = 0 everywhere, every filled channel of the line is NaN
    maps, line = spectrum_stats_host(cube, np.zeros(20, np.uint8), SpectrumStatsParameters(), subtract=True)
    assert not maps['count'].any() and np.isnan(maps['median']).all()
    assert np.array_equal(cases.bits(line), cases.bits(cube))
    maps, line = spectrum_stats_host(cube, filled, SpectrumStatsParameters(exclude_ranges=[(0, 20)]), subtract=True)
    assert not maps['count'].any() and np.isnan(line[filled != 0]).all()


def test_the_order_of_signed_zeros_and_the_median_rule():
    zero = np.float32(0.0)
    spectrum = np.array([zero, -zero, -zero, zero], np.float32).reshape(4, 1)
    maps = spectrum_stats_host(spectrum, np.ones(4), SpectrumStatsParameters(estimator='median_abs'))
    assert cases.bits(maps['min'])[0] == 0x80000000 and cases.bits(maps['max'])[0] == 0
    assert cases.bits(maps['median'])[0] == 0          # (-0 + +0) / 2 = +0
    spectrum = np.array([1, 2, 4, 8, np.nan], np.float32).reshape(5, 1)
    maps = spectrum_stats_host(spectrum, np.ones(5), SpectrumStatsParameters())
    assert maps['median'][0] == 3 and maps['count'][0] == 4
    assert maps['sigma'][0] == np.float32(np.float32(1.5) * cases.TO_RMS)    # |x - 3| = 2 1 1 5


def test_parameter_validation():
    good = SpectrumStatsParameters()
    assert good.estimator == 'mad' and good.outputs == ('median', 'sigma', 'count') and good.min_samples == 1
    assert good.range(7) == (0, 7) and good.stat(7).tolist() == [1] * 7
    assert 'mad' in repr(good)
    for bad in (dict(estimator='mean'), dict(estimator=1), dict(channels=3), dict(channels=(1,)),
                dict(channels=(3, 3)), dict(channels=(-1, 2)), dict(channels=(0, 4097)),
                dict(channels=(True, 3)), dict(channels=(0.5, 3)), dict(exclude_ranges=5),
                dict(exclude_ranges=[(3, 2)]), dict(exclude_ranges=[(False, True)]),
                dict(exclude_ranges=[(1, 2, 3)]), dict(min_samples=0), dict(min_samples=True),
                dict(min_samples=1.5), dict(min_samples='a'), dict(outputs=()), dict(outputs='median'),
                dict(outputs=('median', 'median')), dict(outputs=('mean',)), dict(outputs=(1,)), dict(outputs=3)):
        with pytest.raises(ValueError):
            SpectrumStatsParameters(**bad)
    with pytest.raises(ValueError):
        SpectrumStatsParameters(channels=(0, 9)).range(8)
    with pytest.raises(ValueError):
        SpectrumStatsParameters(exclude_ranges=[(2, 9)]).stat(8)
    with pytest.raises(ValueError):
        good.range(0)
    with pytest.raises(ValueError):
        good.range(4097)
    with pytest.raises(ValueError):
        good.entering(4, np.ones(5))
    params = SpectrumStatsParameters(channels=(1, 6), exclude_ranges=[(2, 3), (4, 8)])
    assert params.stat(8).tolist() == [1, 1, 0, 1, 0, 0, 0, 0]
    assert params.entering(8, [1, 0, 1, 1, 1, 1, 1, 1]).tolist() == [False, False, False, True] + [False] * 4
    cube = np.zeros((4, 2, 2), np.float32)
    with pytest.raises(TypeError):
        spectrum_stats_host(cube.astype(np.float64), np.ones(4), good)
    with pytest.raises(TypeError):
        spectrum_stats_host(cube, np.ones(4), dict())
    with pytest.raises(ValueError):
        spectrum_stats_host(cube[0, 0], np.ones(2), good)
    with pytest.raises(ValueError):
        spectrum_stats_host(cube, np.ones(3), good)
    assert spectrum_stats.OUTPUT_BITS == cases.OUTPUT_BITS
