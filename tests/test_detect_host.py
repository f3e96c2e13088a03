"""The numpy twins of the detection mask (katsdpimager_amd/detect.py: boxcar_host, reblank_host,
threshold_host, prune_host, apply_host, gaussian_taps, smooth_clip_host) against the contract restated
per voxel in plain Python loops (detect_cases.py) on tiny cubes, their known answers, and every
parameter rejection.  No device: the twins are what test_detect_gpu.py holds the kernels to."""
import math

import numpy as np
import pytest

import detect_cases as cases
from katsdpimager_amd import detect, smooth

NAN = np.float32(np.nan)


def _flat(cube):
    return cube.reshape(cube.shape[0], -1)


@pytest.mark.parametrize('C', (1, 2, 3, 8, 9))
def test_boxcar_against_restatement(C):
    for i, plane in enumerate(((1, 1, 1), (1, 3, 5), (2, 3, 4))):
        cube = cases.sprinkled_cube(C, plane, 10 * C + i)
        filled = cases.filled_for(C, C + i)
        mask = cases.random_mask(cube.shape, C + i, values=(1, 2, 255))
        for width in cases.WIDTHS:
            for use_mask in (None, mask):
                for blank in (False, True):
                    got = detect.boxcar_host(cube, filled, width, use_mask, blank)
                    want = cases.restate_boxcar(_flat(cube), filled, width,
                                                None if use_mask is None else _flat(mask), blank)
                    cases.assert_same_bits(_flat(got), want, (C, plane, width, use_mask is None, blank))


def test_boxcar_known_answers():
    C = 9
    filled = np.ones(C, np.uint8)
    cube = cases.sprinkled_cube(C, (1, 4, 5), 3)
    # width 1 without a mask: the cube with what is not finite made 0 (-0 becomes +0: 0.0 + -0.0)
    got = detect.boxcar_host(cube, filled, 1)
    want = np.where(np.isfinite(cube), cube, np.float32(0)) + np.float32(0)
    cases.assert_same_bits(got, want.astype(np.float32))
    assert not np.signbit(got).any() or (got[np.signbit(got)] != 0).all()
    # ... and with blank the NaN are back, exactly where the cube is not finite
    blanked = detect.boxcar_host(cube, filled, 1, blank=True)
    assert np.array_equal(np.isnan(blanked), ~np.isfinite(cube))
    # a delta gives 1 / w in w channels
    delta = np.zeros((C, 1, 1, 1), np.float32)
    delta[4] = 1
    for width in (1, 3, 7):
        got = detect.boxcar_host(delta, filled, width).reshape(C)
        h = width // 2
        want = np.zeros(C, np.float32)
        want[4 - h:4 + h + 1] = np.float32(1.0 / width)
        cases.assert_same_bits(got, want)
    # a mask bit removes exactly that voxel's contribution
    ramp = np.arange(1, C + 1, dtype=np.float32).reshape(C, 1, 1, 1)
    mask = np.zeros(ramp.shape, np.uint8)
    mask[3] = 255
    free = detect.boxcar_host(ramp, filled, 3).reshape(C).astype(np.float64)
    held = detect.boxcar_host(ramp, filled, 3, mask).reshape(C).astype(np.float64)
    difference = (free - held) * 3
    assert np.allclose(difference, [0, 0, 4, 4, 4, 0, 0, 0, 0], atol=1e-5)
    # a width above 2 C sees only zeros beyond the band: every channel is the sum of all, over w
    small = np.array([1, 2, 4], np.float32).reshape(3, 1, 1, 1)
    got = detect.boxcar_host(small, np.ones(3, np.uint8), 7).reshape(3)
    cases.assert_same_bits(got, np.full(3, np.float32(7.0 / 7.0)))
    got = detect.boxcar_host(small, np.ones(3, np.uint8), 31).reshape(3)
    cases.assert_same_bits(got, np.full(3, np.float32(7.0 / 31.0)))
    # an unfilled channel is a zero term and is not written
    hole = np.array([1, 1, 0], np.uint8)
    got = detect.boxcar_host(small, hole, 3).reshape(3)
    cases.assert_same_bits(got, np.array([np.float32(3.0 / 3.0), np.float32(3.0 / 3.0), np.nan], np.float32))


def test_boxcar_sums_in_ascending_order():
    """2^60, 1, -2^60 as float32 values: ascending, (2^60 + 1) - 2^60 = 0 in float64; descending,
    (-2^60 + 1) + 2^60 = 0 as well -- so the triple that tells the orders apart is 1, 2^60, -2^60:
    ascending (1 + 2^60) - 2^60 = 0, descending (-2^60 + 2^60) + 1 = 1."""
    big = np.float32(2.0 ** 60)
    for triple, ascending, descending in (((1.0, big, -big), 0.0, 1.0), ((big, -big, 1.0), 1.0, 0.0)):
        cube = np.array(triple, np.float32).reshape(3, 1, 1, 1)
        got = detect.boxcar_host(cube, np.ones(3, np.uint8), 3).reshape(3)
        assert got[1] == np.float32(ascending / 3.0)
        reverse = 0.0
        for value in triple[::-1]:
            reverse = reverse + float(value)
        assert reverse == descending != ascending
        want = cases.restate_boxcar(cube.reshape(3, 1), np.ones(3, np.uint8), 3)
        cases.assert_same_bits(got.reshape(3, 1), want)


@pytest.mark.parametrize('C', (1, 3, 8))
def test_reblank_and_apply_against_restatement(C):
    plane = (2, 3, 4)
    cube = cases.sprinkled_cube(C, plane, C)
    work = cases.sprinkled_cube(C, plane, C + 50)
    filled = cases.filled_for(C, C)
    got = detect.reblank_host(work, cube, filled)
    cases.assert_same_bits(_flat(got), cases.restate_reblank(_flat(work), _flat(cube), filled))
    on = filled != 0
    assert np.array_equal(np.isnan(got[on]), np.isnan(work[on]) | ~np.isfinite(cube[on]))
    mask = cases.random_mask(cube.shape, C, values=(1, 2, 255))
    for invert in (False, True):
        want = cases.restate_apply(_flat(cube), _flat(mask), filled, invert)
        got = detect.apply_host(cube, mask, filled, invert)
        cases.assert_same_bits(_flat(got), want, (C, invert, 'in place'))
        # out: the unfilled channels are out's own
        target = np.full(cube.shape, np.float32(7), np.float32)
        got = detect.apply_host(cube, mask, filled, invert, out=target)
        want = want.copy()
        want[~on] = 7
        cases.assert_same_bits(_flat(got), want, (C, invert, 'out'))
    kept = detect.apply_host(cube, mask, filled)
    gone = detect.apply_host(cube, mask, filled, invert=True)
    assert (np.isnan(kept[on]) | np.isnan(gone[on])).all()
    both = np.where(mask[on] != 0, kept[on], gone[on])
    cases.assert_same_bits(both, cube[on])


@pytest.mark.parametrize('polarity', cases.POLARITIES)
def test_threshold_against_restatement(polarity):
    for C, P in ((1, 1), (3, 2), (8, 3)):
        work = cases.sprinkled_cube(C, (P, 3, 4), C + P)
        filled = cases.filled_for(C, C)
        before = cases.random_mask(work.shape, C, 0.1, values=(1, 7))
        for G in {1, P}:
            sigma = cases.sigma_table(C, G, G)
            got = detect.threshold_host(work, before, filled, sigma, 1.5, polarity)
            want = cases.restate_threshold(work.reshape(C, P, -1), before.reshape(C, P, -1), filled,
                                           sigma, 1.5, polarity)
            cases.assert_same_bits(got.reshape(C, P, -1), want, (C, P, G))
            # nothing is ever cleared; a byte changes only by becoming 1
            assert (got[before != 0] != 0).all()
            assert ((got == before) | (got == 1)).all()


def test_threshold_known_answers():
    values = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 0.5, -0.5], np.float32)
    work = values.reshape(1, 1, 1, -1)
    filled = np.ones(1, np.uint8)
    empty = np.zeros(work.shape, np.uint8)

    def detected(sigma, polarity, threshold=1.0):
        table = np.array([[sigma]], np.float32)
        return detect.threshold_host(work, empty, filled, table, threshold, polarity).reshape(-1).tolist()
    #                                   +0 -0 +Inf -Inf NaN 1  -1 .5 -.5
    assert detected(0.75, 'positive') == [0, 0, 0, 0, 0, 1, 0, 0, 0]
    assert detected(0.75, 'negative') == [0, 0, 0, 0, 0, 0, 1, 0, 0]
    assert detected(0.75, 'both') == [0, 0, 0, 0, 0, 1, 1, 0, 0]
    # a zero sigma: everything finite and strictly beyond 0 on the side asked for; +-0 never
    assert detected(0.0, 'positive') == [0, 0, 0, 0, 0, 1, 0, 1, 0]
    assert detected(0.0, 'negative') == [0, 0, 0, 0, 0, 0, 1, 0, 1]
    assert detected(0.0, 'both') == [0, 0, 0, 0, 0, 1, 1, 1, 1]
    # a negative cut lets +-0 in; Inf and NaN stay out whatever the cut
    assert detected(-0.75, 'positive') == [1, 1, 0, 0, 0, 1, 0, 1, 1]
    for polarity in cases.POLARITIES:
        assert detected(np.nan, polarity) == [0] * 9
        assert detected(np.inf, polarity) == [0] * 9
    # the cut is one float32 product: 3 * float32(1 / 3) rounds to 1, which 1 is not above
    third = np.float32(1.0) / np.float32(3.0)
    assert np.float32(3.0) * third == np.float32(1.0) and 3.0 * float(third) > 1.0
    assert detected(third, 'positive', 3.0) == [0, 0, 0, 0, 0, 0, 0, 0, 0]
    # unfilled channels are not touched
    got = detect.threshold_host(work, empty, np.zeros(1, np.uint8), np.array([[0.0]], np.float32), 1.0, 'both')
    assert not got.any()


@pytest.mark.parametrize('C', (1, 2, 5, 9, 33))
def test_prune_against_restatement(C):
    mask = cases.run_mask(C, 40, C)
    for min_channels in sorted(m for m in {1, 2, 3, C - 1, C} if 1 <= m <= C):
        got = detect.prune_host(mask.reshape(C, 2, 4, 5), min_channels)
        want = cases.restate_prune(mask, min_channels)
        cases.assert_same_bits(got.reshape(C, 40), want, (C, min_channels))
        assert set(np.unique(got).tolist()) <= {0, 1}
        if min_channels == 1:
            assert np.array_equal(got.reshape(C, 40), (mask != 0).astype(np.uint8))


def test_prune_known_answers():
    def pruned(column, min_channels):
        mask = np.array(column, np.uint8).reshape(-1, 1)
        return detect.prune_host(mask, min_channels).reshape(-1).tolist()
    # runs of length 1, min - 1 and min, at both ends of the band
    assert pruned([1, 0, 1, 1, 0, 1, 1, 1], 3) == [0, 0, 0, 0, 0, 1, 1, 1]
    assert pruned([1, 1, 1, 0, 1, 1, 0, 1], 3) == [1, 1, 1, 0, 0, 0, 0, 0]
    assert pruned([1, 1, 0, 1], 2) == [1, 1, 0, 0]
    assert pruned([1, 0, 1, 1], 2) == [0, 0, 1, 1]
    # an all-zero channel (an unfilled one) splits a run
    assert pruned([1, 1, 0, 1, 1], 3) == [0, 0, 0, 0, 0]
    assert pruned([1, 1, 0, 1, 1], 2) == [1, 1, 0, 1, 1]
    # any nonzero byte is set; what stays becomes 1
    assert pruned([2, 255, 0, 9], 2) == [1, 1, 0, 0]
    assert pruned([2, 255, 0, 9], 1) == [1, 1, 0, 1]
    assert pruned([1, 1, 1, 1], 4) == [1, 1, 1, 1]
    assert pruned([0, 1, 1, 1], 4) == [0, 0, 0, 0]


@pytest.mark.parametrize('fwhm', (0.5, 1.0, 3.0, 6.0, 12.5))
def test_gaussian_taps(fwhm):
    for truncate in (2.0, 3.0):
        radius, taps = detect.gaussian_taps(fwhm, truncate)
        sigma = fwhm / (2.0 * math.sqrt(2.0 * math.log(2.0)))
        assert radius == math.ceil(truncate * sigma)
        D = 2 * radius + 1
        assert taps.dtype == np.float32 and taps.shape == (D * D,)
        # one float32 rounding per tap, each of a value of at most 1
        assert abs(float(taps.astype(np.float64).sum()) - 1.0) <= taps.size * 2.0 ** -25
        square = taps.reshape(D, D)
        assert np.array_equal(square, square.T) and np.array_equal(square, square[::-1, ::-1])
        assert square[radius, radius] == square.max()
        ratio = float(square[radius, radius + 1]) / float(square[radius, radius])
        assert abs(ratio - math.exp(-0.5 / sigma ** 2)) < 1e-6


def test_gaussian_taps_edges():
    radius, taps = detect.gaussian_taps(0)
    assert radius == 0 and taps.dtype == np.float32 and taps.tolist() == [1.0]
    assert detect.gaussian_taps(3)[0] == 4 and detect.gaussian_taps(6)[0] == 8
    sigma_16 = 16 / 3.0 * (2.0 * math.sqrt(2.0 * math.log(2.0)))
    assert detect.gaussian_taps(sigma_16 * 0.999)[0] == smooth.MAX_RADIUS
    for bad in (sigma_16 * 1.07, 100.0, -1.0, float('nan'), float('inf'), 'wide', None):
        with pytest.raises(ValueError):
            detect.gaussian_taps(bad)
    for bad in (0.0, -1.0, float('nan'), float('inf'), 'x'):
        with pytest.raises(ValueError):
            detect.gaussian_taps(3.0, bad)


def test_parameter_rejections():
    P = detect.SmoothClipParameters
    ok = P()
    assert ok.spatial_fwhm == (0.0, 3.0, 6.0) and ok.spectral_widths == (1, 3, 7)
    assert ok.threshold == 5.0 and ok.polarity == 'positive' and ok.estimator == 'median_abs'
    assert ok.pool_polarizations is True and ok.border == 0 and ok.replace is True
    assert ok.min_channels == 1 and ok.truncate == 3.0
    assert 'spatial_fwhm=(0.0, 3.0, 6.0)' in repr(ok)
    bad = [
        dict(spatial_fwhm=()), dict(spatial_fwhm=None), dict(spatial_fwhm='3'), dict(spatial_fwhm=3),
        dict(spatial_fwhm=(-1,)), dict(spatial_fwhm=(float('nan'),)), dict(spatial_fwhm=(14,)),
        dict(spatial_fwhm=(True,)), dict(spatial_fwhm=('a',)),
        dict(spectral_widths=()), dict(spectral_widths=None), dict(spectral_widths='3'),
        dict(spectral_widths=(2,)), dict(spectral_widths=(0,)), dict(spectral_widths=(33,)),
        dict(spectral_widths=(3.5,)), dict(spectral_widths=(True,)), dict(spectral_widths=(-3,)),
        dict(threshold=0), dict(threshold=-1), dict(threshold=float('nan')), dict(threshold=float('inf')),
        dict(threshold=1e39), dict(threshold=1e-50), dict(threshold='x'), dict(threshold=None),
        dict(polarity='up'), dict(polarity=0), dict(polarity=None),
        dict(estimator='rms'), dict(estimator=None),
        dict(pool_polarizations=1), dict(pool_polarizations=None),
        dict(border=-1), dict(border=1.5), dict(border=True),
        dict(replace=1), dict(replace=None),
        dict(min_channels=0), dict(min_channels=1.5), dict(min_channels=True), dict(min_channels=4097),
        dict(truncate=0), dict(truncate=float('inf')), dict(truncate='x'),
    ]
    for keywords in bad:
        with pytest.raises(ValueError):
            P(**keywords)
    # a truncate that takes FWHM 6 past radius 16
    with pytest.raises(ValueError):
        P(truncate=7.0)
    assert P(spatial_fwhm=[6], spectral_widths=[31], truncate=6.0).spectral_widths == (31,)
    # the shape a cube must have
    with pytest.raises(ValueError):
        P(min_channels=5).check_shape((4, 1, 8, 8))
    with pytest.raises(ValueError):
        P(border=4).check_shape((4, 1, 8, 8))
    P(border=3, min_channels=4).check_shape((4, 1, 8, 8))


def test_twin_argument_rejections():
    cube = np.zeros((3, 1, 2, 2), np.float32)
    filled = np.ones(3, np.uint8)
    mask = np.zeros(cube.shape, np.uint8)
    sigma = np.ones((3, 1), np.float32)
    with pytest.raises(TypeError):
        detect.boxcar_host(cube.astype(np.float64), filled, 3)
    for width in (2, 0, 33, 1.5, True):
        with pytest.raises(ValueError):
            detect.boxcar_host(cube, filled, width)
    with pytest.raises(ValueError):
        detect.boxcar_host(cube, filled[:2], 3)
    with pytest.raises(ValueError):
        detect.boxcar_host(cube, filled, 3, mask[:2])
    with pytest.raises(TypeError):
        detect.boxcar_host(cube, filled, 3, mask.astype(np.float32))
    with pytest.raises(ValueError):
        detect.reblank_host(cube[:2], cube, filled)
    for threshold in (0, -1, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            detect.threshold_host(cube, mask, filled, sigma, threshold)
    with pytest.raises(ValueError):
        detect.threshold_host(cube, mask, filled, sigma, 5, 'up')
    with pytest.raises(ValueError):
        detect.threshold_host(cube, mask, filled, np.ones((3, 2), np.float32), 5)
    with pytest.raises(ValueError):
        detect.threshold_host(cube, mask, filled, sigma.astype(np.float64), 5)
    for min_channels in (0, 4, True, 1.5):
        with pytest.raises(ValueError):
            detect.prune_host(mask, min_channels)
    with pytest.raises(ValueError):
        detect.apply_host(cube, mask[:2], filled)
    with pytest.raises(TypeError):
        detect.smooth_clip_host(cube, filled, None)
    with pytest.raises(ValueError):
        detect.smooth_clip_host(cube[:, 0], filled, detect.SmoothClipParameters())


def test_finder_order_and_replacement():
    """smooth_clip_host is the stated sequence of the twins: restated here step by step for two
    FWHMs and two widths, with and without replacement; and `replace` changes the result where a
    bright source would be smeared into a halo."""
    from katsdpimager_amd import cube_stats
    cube, filled, region = cases.finder_cube()
    cube = np.ascontiguousarray(cube[:, :, 4:28, 4:36])
    region = np.ascontiguousarray(region[4:28, 4:36])
    C = cube.shape[0]
    masks = {}
    for replace in (True, False):
        params = detect.SmoothClipParameters(spatial_fwhm=(0, 3), spectral_widths=(1, 3), threshold=3.5,
                                             replace=replace, min_channels=2, estimator='mad',
                                             pool_polarizations=False, border=2)
        mask = np.zeros(cube.shape, np.uint8)
        stats = cube_stats.CubeStatsParameters(estimator='mad', border=2, pool_polarizations=False)
        for fwhm in (0, 3):
            radius, taps = detect.gaussian_taps(fwhm)
            for width in (1, 3):
                work = detect.boxcar_host(cube, filled, width, mask if replace else None, blank=fwhm == 0)
                if fwhm:
                    work = smooth.cube_smooth_host(work, filled, np.full(C, radius, np.int32),
                                                   np.tile(taps, (C, 1)))
                    work = detect.reblank_host(work, cube, filled)
                assert np.array_equal(np.isnan(work[filled != 0]), ~np.isfinite(cube[filled != 0]))
                sigma = cube_stats.cube_stats_host(work, filled, stats, region).sigma
                mask = detect.threshold_host(work, mask, filled, sigma, 3.5, 'positive')
        mask = detect.prune_host(mask, 2)
        got = detect.smooth_clip_host(cube, filled, params, region)
        assert np.array_equal(got, mask)
        assert got.any() and not got[filled == 0].any() and not got[~np.isfinite(cube)].any()
        masks[replace] = got
    assert not np.array_equal(masks[True], masks[False])
    assert masks[True].sum() < masks[False].sum()


def test_faint_source_needs_the_kernels():
    """What seed and amplitude of the demonstration were fixed for: the source's peak is below the cut
    of every voxel, the per-voxel clip finds nothing at the source, the full kernel set finds its
    centre and nothing away from it."""
    from katsdpimager_amd import cube_stats
    cube, filled = cases.faint_cube()
    sigma = cube_stats.cube_stats_host(cube, filled, cube_stats.CubeStatsParameters()).sigma
    assert cases.FAINT_AMPLITUDE < cases.FAINT_THRESHOLD * sigma.min()
    single = detect.smooth_clip_host(cube, filled, detect.SmoothClipParameters(
        spatial_fwhm=(0,), spectral_widths=(1,), threshold=cases.FAINT_THRESHOLD))
    full = detect.smooth_clip_host(cube, filled, detect.SmoothClipParameters(threshold=cases.FAINT_THRESHOLD))
    cases.assert_faint_source(single, full)
