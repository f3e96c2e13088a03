"""Cube plane statistics on the device (csrc/cube_stats.hip through cube_stats.CubeStats) against the
numpy twin (cube_stats.cube_stats_host, tested on its own in test_cube_stats_host.py): all five
outputs bit for bit, whatever the layout, the kernel form and the launch geometry.  Every cube sits
inside a buffer of sentinels that must be unchanged byte for byte afterwards: the cube is never
written.

Layouts: the channel pitch padded by 0, 3 and 4 floats, and once more starting 1 float into the
buffer.  With buffers that are 16-byte aligned, pads 0 and 4 at offset 0 get the 16-byte loads when W
and P * H * W are multiples of 4 floats; pad 3 (unless P * H * W + 3 is a multiple of 4, which it is for
none of the planes with W a multiple of 4) and offset 1 get one element a load, and so does every
plane whose W is no multiple of 4.  cube_stats_cases.form says which."""
import numpy as np
import pytest

import cube_stats_cases as cases
from helpers import context_queue

pytestmark = pytest.mark.gpu

#: (the layouts, the padded cube and the run over the layouts are shared with test_cube_band_gpu.py)
_PaddedCube = cases.PaddedCube
_check = cases.check


@pytest.mark.parametrize('C', [1, 5, 70])
def test_device_against_twin(C):
    """Every plane on every layout, the mode rotating with the plane; some channels unfilled."""
    ctx, q = context_queue()
    forms, groups = set(), 0
    all_modes = cases.modes()
    planes = cases.PLANES + (cases.MULTI_BLOCK_PLANE, cases.ONE_PIXEL_PLANE)
    for i, plane in enumerate(planes):
        pool, estimator, border, region = all_modes[(5 * i + C) % len(all_modes)]
        if plane == cases.ONE_PIXEL_PLANE:
            border, region = 2, 'none'
        elif plane == cases.MULTI_BLOCK_PLANE:
            region = 'sparse' if C == 5 else 'none'
        elif not cases.border_fits(border, plane):
            border = 0
        values = 'non_finite' if i % 2 else 'noise_like'
        cube, filled, mask = cases.make_case(C, plane, 1000 * C + i, values, region)
        keywords = dict(estimator=estimator, border=border, pool_polarizations=pool)
        twin = _check(ctx, q, cube, filled, keywords, mask, forms, (C, plane), device_region=i % 3 == 0)
        groups += int((twin.count > 0).sum())
        assert (twin.count[filled == 0] == 0).all()
    assert forms == {'scalar', 'vector'}
    assert groups >= 4 * C


def test_every_mode():
    """Pooled and per polarization, both estimators, border 0 and 1, no region, a full, a sparse and
    an empty one: all 32, on a plane of either kernel form, with NaN and Inf in the data and one
    channel all NaN."""
    ctx, q = context_queue()
    forms, empty = set(), 0
    for plane in ((2, 7, 9), (4, 8, 12)):
        for n, (pool, estimator, border, region) in enumerate(cases.modes()):
            cube, filled, mask = cases.make_case(3, plane, 50 + n, 'non_finite', region, sprinkle=False)
            filled[:] = 1
            keywords = dict(estimator=estimator, border=border, pool_polarizations=pool)
            twin = _check(ctx, q, cube, filled, keywords, mask, forms, (plane, pool, estimator, border, region),
                          layouts=((0, 0), (3, 0)), device_region=n % 2 == 0)
            assert (twin.count[2] == 0).all() and np.isnan(twin.sigma[2]).all()
            empty += int(region == 'empty' and not twin.count.any())
            assert region == 'empty' or twin.count[:2].all()
    assert forms == {'scalar', 'vector'} and empty == 16


@pytest.mark.parametrize('values', sorted(cases.VALUE_SETS))
def test_value_sets(values):
    """Each value set under both estimators, pooled and per polarization; the larger plane holds all
    510 values of every_exponent in a group."""
    ctx, q = context_queue()
    forms = set()
    for plane in ((2, 7, 9), (2, 33, 64)):
        for estimator in cases.ESTIMATORS:
            for pool in (True, False):
                cube, filled, mask = cases.make_case(4, plane, 7, values, sprinkle=values == 'noise_like')
                twin = _check(ctx, q, cube, filled, dict(estimator=estimator, pool_polarizations=pool),
                              mask, forms, (values, plane, estimator, pool), layouts=((0, 0), (0, 1)))
                on = filled != 0
                if values == 'non_finite':
                    on[-1] = False
                    assert not twin.count[-1].any()
                assert twin.count[on].all()
                if values == 'offset' and plane[1] == 33:
                    # what 'mad' is for: the scatter, not the offset
                    assert ((twin.sigma[on] < 2) if estimator == 'mad' else (twin.sigma[on] > 140)).all()
    assert forms == {'scalar', 'vector'}


def test_ranges_and_tiny_groups():
    """A range inside the band; groups of exactly 1, 2 and 3 samples, and 2, 4 and 6 pooled; a border
    that leaves one pixel."""
    ctx, q = context_queue()
    forms = set()
    for channels in ((0, 1), (2, 5), (6, 7), (1, 7)):
        cube, filled, mask = cases.make_case(7, (2, 7, 9), 21)
        twin = _check(ctx, q, cube, filled, dict(channels=channels, estimator='mad'), mask, forms,
                      (channels,))
        outside = np.ones(7, bool)
        outside[channels[0]:channels[1]] = False
        assert not twin.count[outside].any() and twin.count[~outside & (filled != 0)].all()
    counts = set()
    for estimator in cases.ESTIMATORS:
        for k in (1, 2, 3):
            for plane, pool in (((1, 7, 9), True), ((2, 8, 12), True), ((2, 8, 12), False)):
                cube, filled, mask = cases.make_case(3, plane, 30 + k, region=k, sprinkle=False)
                twin = _check(ctx, q, cube, filled, dict(estimator=estimator, pool_polarizations=pool),
                              mask, forms, (estimator, k, plane, pool))
                counts.update(int(n) for n in twin.count[filled != 0].reshape(-1))
        cube, filled, mask = cases.make_case(2, cases.ONE_PIXEL_PLANE, 40, sprinkle=False)
        twin = _check(ctx, q, cube, filled, dict(estimator=estimator, border=2, pool_polarizations=False),
                      mask, forms, (estimator, 'one pixel'))
        assert (twin.count[filled != 0] == 1).all()
    assert counts == {1, 2, 3, 4, 6} and forms == {'scalar', 'vector'}


@pytest.mark.parametrize('border', [0.0, 0.07])
def test_continuity_with_noise_est(border):
    """On finite planes, pooled, without region: sigma under 'median_abs' is what clean.NoiseEst returns
    for the same plane, by bits -- border 0, and one that border_pixels maps to a pixel count above 0."""
    from katsdpimager_amd import clean, cube_stats
    from katsdpimager_amd.image_plane import border_pixels
    ctx, q = context_queue()
    for plane in ((1, 33, 65), (2, 70, 132), (4, 40, 48)):
        P, H, W = plane
        pixels = border_pixels(border, plane)
        assert (pixels > 0) == (border > 0)
        cube, filled, _ = cases.make_case(3, plane, 60 + P, 'noise_like', sprinkle=False)
        filled[:] = 1
        params = cube_stats.CubeStatsParameters(border=pixels)
        source = _PaddedCube(ctx, q, cube, 0, 0)
        got = cube_stats.CubeStatsTemplate(ctx, params).instantiate(q, cube.shape)(source.array, filled=filled)
        single = clean.NoiseEstTemplate(ctx, np.float32, P).instantiate(q, plane, border)
        single.ensure_all_bound()
        assert single.border_pixels == pixels
        for c in range(3):
            single.buffer('dirty').set(q, cube[c])
            want = single()
            assert want.dtype == np.float32 and np.isfinite(want)
            assert cases.bits(got.sigma[c, 0]) == cases.bits(want), (plane, c, got.sigma[c, 0], want)


def test_driver_smooth_measure_moments():
    """put(beam=), CubeSmooth, op(smoothed, update_noise=True), Moments with clip_sigma -- which raised
    ValueError before anything could measure the smoothed planes -- and moment 0 against moments_host
    fed the twin's noise, by bits."""
    from katsdpimager_amd import cube, cube_stats, smooth
    from katsdpimager_amd.beam import Beam
    ctx, q = context_queue()
    C, P, H, W = 6, 2, 21, 24
    rng = np.random.default_rng(12)
    frequencies = 1.4e9 * (1.0 + 0.05 * np.arange(C) / (C - 1))
    beams = [Beam(1.0, 2.4 * frequencies[0] / f, 1.8 * frequencies[0] / f, 0.6) for f in frequencies]
    data = rng.normal(0.0, 1.0, (C, P, H, W)).astype(np.float32)
    data[:, :, 8:12, 9:14] += 6.0                               # something above the cut
    source = cube.SpectralCube(ctx, q, frequencies, P, (H, W))
    for c in (0, 1, 2, 3, 5):
        source.put(c, data[c], 1.0, beam=beams[c])
    smoother = smooth.CubeSmoothTemplate(ctx, smooth.CommonBeamParameters()).instantiate(q, source.shape)
    smoothed = smoother(source)
    assert np.isnan(smoothed.noise[[1, 2, 3, 4, 5]]).all()
    parameters = cube.MomentParameters((0,), axis='frequency', clip_sigma=3)
    moments = cube.MomentsTemplate(ctx, parameters).instantiate(q, smoothed.shape)
    with pytest.raises(ValueError, match='no noise recorded'):
        moments(smoothed)
    params = cube_stats.CubeStatsParameters()
    op = cube_stats.CubeStatsTemplate(ctx, params).instantiate(q, smoothed.shape)
    result = op(smoothed, update_noise=True)
    held = smoothed.get()
    twin = cube_stats.cube_stats_host(held, smoothed.filled, params)
    cases.assert_same(result, twin)
    on = smoothed.filled != 0
    assert np.array_equal(cases.bits(smoothed.noise[on]), cases.bits(twin.sigma[on, 0]))
    assert np.isnan(smoothed.noise[4]) and np.isfinite(smoothed.noise[on]).all()
    m0 = moments(smoothed)[0].get(q)
    want = cube.moments_host(held, frequencies, parameters.cut_table(C, twin.sigma[:, 0], smoothed.filled),
                             smoothed.filled, parameters)[0]
    assert np.array_equal(cases.bits(m0), cases.bits(want)) and np.isfinite(m0).any()
    # a second call with a range leaves the channels outside it alone; per-plane results cannot be recorded
    smoothed.noise[:] = 5.0
    ranged = cube_stats.CubeStatsTemplate(ctx, cube_stats.CubeStatsParameters(channels=(1, 4))).instantiate(q, smoothed.shape)
    ranged(smoothed, region=np.ones((H, W), bool), update_noise=True)
    assert (smoothed.noise[[0, 4, 5]] == 5.0).all()
    assert np.array_equal(cases.bits(smoothed.noise[1:4]), cases.bits(twin.sigma[1:4, 0]))
    per_plane = cube_stats.CubeStatsTemplate(ctx, cube_stats.CubeStatsParameters(pool_polarizations=False)).instantiate(q, smoothed.shape)
    with pytest.raises(ValueError, match='pool_polarizations'):
        per_plane(smoothed, update_noise=True)
    assert per_plane(smoothed).sigma.shape == (C, P)
    # refusals of the call
    with pytest.raises(ValueError):
        op(smoothed, filled=smoothed.filled)
    with pytest.raises(ValueError):
        op(smoothed.array)
    with pytest.raises(ValueError, match='SpectralCube'):
        op(smoothed.array, filled=smoothed.filled, update_noise=True)
    with pytest.raises(TypeError):
        op(held, filled=smoothed.filled)
    with pytest.raises(ValueError):
        op(smoothed, region=np.ones((H, W + 1), np.uint8))
    with pytest.raises(TypeError):
        op(smoothed, region=np.ones((H, W), np.float32))
    with pytest.raises(ValueError):
        cube_stats.CubeStatsTemplate(ctx, params).instantiate(q, (C, P, H))
    with pytest.raises(ValueError, match='border'):
        cube_stats.CubeStatsTemplate(ctx, cube_stats.CubeStatsParameters(border=11)).instantiate(q, smoothed.shape)


def test_argument_errors_return_their_codes_and_write_nothing():
    import ctypes
    from katsdpimager_amd import accel, _lib
    ctx, q = context_queue()
    lib = _lib.lib()
    C, P, H, W = 4, 2, 4, 8
    M = P * H * W
    memory = accel.DeviceArray(ctx, (C * M,), np.float32)
    memory.set(q, np.full(memory.shape, 7.0, np.float32))
    words = lib.kimg_cube_stats_scratch_bytes(C, P) // 4
    assert words > 0 and lib.kimg_cube_stats_scratch_bytes(C, 1) > 0
    for bad in ((0, 1), (4097, 1), (4, 0), (4, 65536)):
        assert lib.kimg_cube_stats_scratch_bytes(*bad) == 0
    scratch = accel.DeviceArray(ctx, (words,), np.uint32)
    scratch.set(q, np.full(words, 9, np.uint32))
    out = accel.DeviceArray(ctx, (5, C * P), np.uint32)
    out.set(q, np.full(out.shape, 9, np.uint32))
    ones = (ctypes.c_uint8 * 4097)(*([1] * 4097))
    outs = [out.ptr + 4 * C * P * i for i in range(5)]
    good = dict(cube=memory.ptr, pitch=M, C=C, P=P, H=H, W=W, filled=ctypes.cast(ones, ctypes.c_void_p),
                first=0, stop=C, pool=0, estimator=0, border=0, region=None, scratch=scratch.ptr,
                count=outs[0], min=outs[1], max=outs[2], median=outs[3], sigma=outs[4])
    bad = [(dict([(name, None)]), cases.EINVAL)
           for name in ('cube', 'filled', 'scratch', 'count', 'min', 'max', 'median', 'sigma')]
    bad += [
        (dict(C=0), cases.EINVAL), (dict(C=4097), cases.EINVAL), (dict(P=0), cases.EINVAL),
        (dict(H=0), cases.EINVAL), (dict(W=-8), cases.EINVAL),
        (dict(first=-1), cases.EINVAL), (dict(first=2, stop=2), cases.EINVAL), (dict(stop=C + 1), cases.EINVAL),
        (dict(estimator=2), cases.EINVAL), (dict(estimator=-1), cases.EINVAL),
        (dict(border=-1), cases.EINVAL), (dict(border=2), cases.EINVAL), (dict(border=2 ** 30), cases.EINVAL),
        (dict(cube=memory.ptr + 2), cases.EINVAL), (dict(scratch=scratch.ptr + 4), cases.EINVAL),
        (dict(sigma=outs[4] + 2), cases.EINVAL),
        (dict(pitch=M - 1), cases.EINVAL), (dict(pitch=2 ** 61), cases.EINVAL),
        (dict(P=2 ** 31 - 1, H=2 ** 31 - 1, W=2 ** 31 - 1, pitch=2 ** 62), cases.EINVAL),
        # a group of 2^32 elements, pooled and per plane; more groups a channel than a launch has rows
        (dict(P=4, H=2 ** 15, W=2 ** 15, pitch=2 ** 32, C=1, stop=1, pool=1), cases.EUNSUPPORTED),
        (dict(P=1, H=2 ** 16, W=2 ** 16, pitch=2 ** 32, C=1, stop=1), cases.EUNSUPPORTED),
        (dict(P=65536, H=1, W=1, pitch=65536, C=1, stop=1), cases.EUNSUPPORTED),
    ]
    for change, code in bad:
        a = dict(good, **change)
        got = lib.kimg_cube_stats(a['cube'], a['pitch'], a['C'], a['P'], a['H'], a['W'], a['filled'],
                                  a['first'], a['stop'], a['pool'], a['estimator'], a['border'],
                                  a['region'], a['scratch'], a['count'], a['min'], a['max'], a['median'],
                                  a['sigma'], q.handle)
        assert got == code, (change, got)
    assert (memory.get(q) == 7.0).all() and (scratch.get(q) == 9).all() and (out.get(q) == 9).all()
