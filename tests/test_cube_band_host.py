"""The long-band cases of cube_band_cases.py on the host: every self-check of the case module (each
case reaches the code path it is there for), the numpy twins against their independent restatements
on the bands of up to 97 channels, and each long-band twin once.  No GPU."""
import numpy as np
import pytest

import band_cases
import cube_band_cases as cases
import cube_smooth_cases
import cube_stats_cases
import detect_cases
import link_cases
from katsdpimager_amd import cube_stats, detect, link, smooth


def test_filled_patterns():
    cases.check_filled()


# ---- smoothing ---------------------------------------------------------------------------------------

def test_smooth_coverage():
    cases.check_smooth()


@pytest.mark.parametrize('C', cases.SMOOTH_CHANNELS)
def test_smooth_twin_against_direct(C):
    checked = 0
    for name, plane, cube, filled, radius, taps in cases.smooth_short_cases(C):
        twin = smooth.cube_smooth_host(cube, filled, radius, taps)
        checked += cube_smooth_cases.assert_within_bound(twin, cube, filled, radius, taps, name)
        assert np.isnan(twin[filled == 0]).all(), name
    assert checked > 100 * C


def test_smooth_twin_at_the_limit():
    name, plane, cube, filled, radius, taps = cases.smooth_limit_cases()[0]
    twin = smooth.cube_smooth_host(cube, filled, radius, taps)
    assert cube_smooth_cases.assert_within_bound(twin, cube, filled, radius, taps, name) > 200000


# ---- plane statistics --------------------------------------------------------------------------------

def test_stats_coverage():
    cases.check_stats()


def _against_independent(name, cube, filled, keywords, region):
    params = cube_stats.CubeStatsParameters(**keywords)
    got = cube_stats.cube_stats_host(cube, filled, params, region)
    first, stop = params.range(cube.shape[0])
    want, exact = cube_stats_cases.independent(cube, filled, first, stop, params.estimator, params.border,
                                               params.pool_polarizations, region)
    assert np.array_equal(got.count, want['count']), name
    some = got.count > 0
    for field in cube_stats_cases.FIELDS[1:]:
        a, b, e = getattr(got, field), want[field], exact[field]
        assert np.array_equal(cube_stats_cases.bits(a)[e], cube_stats_cases.bits(b)[e]), (name, field)
        assert (a[~e & some] == b[~e & some]).all(), (name, field)
    quiet = cases.stats_quiet_groups(cube.shape, filled, keywords)
    # (the value set non_finite makes the last channel all NaN: its groups are empty too)
    assert not got.count[quiet].any() and got.count[:-1][~quiet[:-1]].all(), name
    assert (cube_stats_cases.bits(got.sigma)[quiet] == cube_stats_cases.QUIET_NAN).all(), name


@pytest.mark.parametrize('C', cases.STATS_SEAM_CHANNELS)
def test_stats_twin_on_the_seams(C):
    for case in cases.stats_seam_cases(C):
        _against_independent(*case)


def test_stats_twin_on_the_slot_counts():
    for case in cases.stats_slot_cases():
        if case[1].shape[0] <= 97:
            _against_independent(*case)


def test_stats_twin_at_the_limit():
    name, cube, filled, keywords, region = cases.stats_limit_cases()[0]
    got = cube_stats.cube_stats_host(cube, filled, cube_stats.CubeStatsParameters(**keywords), region)
    quiet = cases.stats_quiet_groups(cube.shape, filled, keywords)
    assert quiet.sum() == 3 * len(cases.STATS_LIMIT_UNFILLED) and not got.count[quiet].any()
    assert got.count[:-1][~quiet[:-1]].all()        # (non_finite's last channel is all NaN)


# ---- detection mask ----------------------------------------------------------------------------------

def test_detect_coverage():
    cases.check_detect()


@pytest.mark.parametrize('C', cases.PRUNE_CHANNELS)
def test_prune_masks(C):
    walks = set()
    for min_channels in cases.prune_minima(C):
        mask = cases.prune_mask(C, min_channels)
        pruned = detect.prune_host(mask, min_channels)
        walks.add(cases.check_prune(C, min_channels, mask, pruned))
        if min_channels <= 33 and C == 257:
            detect_cases.assert_same_bits(pruned, detect_cases.restate_prune(mask, min_channels))
    assert max(clear for clear, _ in walks) >= 255 and max(rewrite for _, rewrite in walks) >= 255


def test_detect_twins_against_restatements_at_97():
    C = 97
    filled = band_cases.straddle(C)
    cube, mask = cases.boxcar_case(C, (1, 3, 5), 5)
    flat, flat_mask = cube.reshape(C, -1), mask.reshape(C, -1)
    for width, with_mask, blank in ((31, True, True), (7, False, False)):
        got = detect.boxcar_host(cube, filled, width, mask if with_mask else None, blank)
        want = detect_cases.restate_boxcar(flat, filled, width, flat_mask if with_mask else None, blank)
        detect_cases.assert_same_bits(got.reshape(C, -1)[filled != 0], want[filled != 0], width)
    for polarity in detect_cases.POLARITIES:
        work, mask, sigma = cases.threshold_case(C, filled, 6, polarity)
        got = detect.threshold_host(work, mask, filled, sigma, cases.THRESHOLD, polarity)
        want = detect_cases.restate_threshold(work.reshape(C, 3, -1), mask.reshape(C, 3, -1), filled, sigma,
                                              cases.THRESHOLD, polarity)
        detect_cases.assert_same_bits(got.reshape(C, 3, -1), want, polarity)
        cases.check_threshold(C, filled, work, mask, sigma, got, polarity)
    other = detect_cases.sprinkled_cube(C, (3, 3, 5), 8)
    detect_cases.assert_same_bits(detect.reblank_host(other, work, filled).reshape(C, -1),
                                  detect_cases.restate_reblank(other.reshape(C, -1), work.reshape(C, -1), filled))
    for invert in (False, True):
        detect_cases.assert_same_bits(detect.apply_host(work, mask, filled, invert).reshape(C, -1),
                                      detect_cases.restate_apply(work.reshape(C, -1), mask.reshape(C, -1), filled, invert))


def test_detect_twins_at_the_limit():
    C = cases.MAX_CHANNELS
    filled = band_cases.limit_mask(C)
    cube, mask = cases.boxcar_case(C, (1, 5, 12), 9)
    got = detect.boxcar_host(cube, filled, 31, mask, True)
    assert np.isnan(got[filled == 0]).all() and np.isfinite(got[filled != 0]).any()
    work, mask, sigma = cases.threshold_case(C, filled, 10, 'positive')
    result = detect.threshold_host(work, mask, filled, sigma, cases.THRESHOLD, 'positive')
    cases.check_threshold(C, filled, work, mask, sigma, result, 'positive')
    assert cases.threshold_rows(C, filled)[-1] == C - 2
    pruned = detect.prune_host(cases.prune_mask(1025, 1025), 1025)
    # (at min_channels = C only whole columns are left)
    assert pruned.all(axis=0).sum() == pruned.any(axis=0).sum() >= 2


# ---- linking -----------------------------------------------------------------------------------------

def test_link_seams_split_and_bridge():
    results = {}
    for C in cases.LINK_SEAM_CHANNELS:
        for name, mask, cube, filled, reach, minima in cases.link_seam_cases(C):
            labels, N0 = link.link_host(mask, filled, *reach)
            results[name] = cases.check_link_seam(name, labels, filled)
            if C <= 97 and name[1] == (3, 3, 5) and reach[0] == 1:
                want, want_N0, rows = link_cases.restate(mask, filled, cube, *reach)
                assert N0 == want_N0, name
                link_cases.assert_same_bits(labels, want, name)
                exact = bool(np.all(cube[np.isfinite(cube)] == np.round(cube[np.isfinite(cube)])))
                link_cases.assert_table(link.measure_host(labels, cube, filled), rows, name, exact_sums=exact)
    cases.check_link_seams(results)


def test_link_scan_coverage():
    cases.check_link_scan()


@pytest.mark.parametrize('C,plane', cases.LINK_SCAN_SHAPES)
def test_link_scan_twins(C, plane):
    for name, mask, filled, reach in cases.link_scan_cases(C, plane):
        labels, N0 = link.link_host(mask, filled, *reach)
        cases.check_link_scan_case(name, mask, filled, labels, N0)
        if name == ('sparse', 'filled'):
            table = link.measure_host(labels, link_cases.integer_cube(mask.shape, 3), filled)
            y, x = cases.column_pixel(plane, 0)
            s = labels[0, 0, y, x] - 1
            assert table['c0'][s] == 0 and table['c1'][s] == C - 1 and table['voxels'][s] >= C


def test_filter_tiles():
    mask = cases.filter_runs_mask()
    filled = np.ones(mask.shape[0], np.uint8)
    labels, N0 = link.link_host(mask, filled, 0, 1)
    table = link.measure_host(labels, link_cases.integer_cube(mask.shape, 4), filled)
    assert cases.check_filter_runs(table) == N0
    for N0 in (1024, 1025):
        mask = cases.filter_exact_mask(N0)
        labels, count = link.link_host(mask, np.ones(41, np.uint8), 0, 0)
        table = link.measure_host(labels, link_cases.integer_cube(mask.shape, 5), np.ones(41, np.uint8))
        assert count == N0 == len(table)
        assert cases.filter_keep(table, (1, 1, 1)).all() and not cases.filter_keep(table, (2, 1, 1)).any()
