"""RFI flagging without a device: the parameters, the numpy twin of the device operator
(rfiflag.rfiflag_host, the executable form of the contract in include/kimg.h) on hand-made planes
whose answer is known by construction and against the contract as plain loops
(rfiflag_cases.by_loops), the C entry point's argument checks, and the loader's keyword.

The hand-made planes have z = 1 everywhere (weight 1 under a visibility of 1) but where a sample is
`put`, so that the level is 1 or a little above it and an ordinary sample adds about 0 to a window;
with the default threshold 6 and rho 1.5 the per-sample thresholds of windows of 1, 2, 4, 8 and 16
samples are 6, 4, 2.67, 1.78 and 1.19 times the level."""
import ctypes
import os
import re

import numpy as np
import pytest

import band_cases as bands
import rfiflag_cases as cases
from katsdpimager_amd import loader, rfiflag
from katsdpimager_amd.rfiflag import RFIFlagParameters, rfiflag_host

EINVAL, EUNSUPPORTED, EWORKSPACE = -10001, -10002, -10003


def _run(vis, weights, ids, params):
    """The twin, checked against the loops; (flags, level, counts) and the weights checked against
    the flags."""
    got = rfiflag_host(vis, weights, ids, params)
    cases.assert_same(got, cases.by_loops(vis, weights, ids, params))
    new, flags, level, counts = got
    assert np.array_equal(new.view(np.uint32)[flags == 0], weights.view(np.uint32)[flags == 0])
    assert not new.view(np.uint32)[flags == 1].any()
    return flags, level, counts


def _only(flags, where):
    want = np.zeros_like(flags)
    for at in where:
        want[at] = 1
    return np.array_equal(flags, want)


# ---- parameters -------------------------------------------------------------------------------------
def test_parameters_their_mask_and_their_factors():
    p = RFIFlagParameters()
    assert (p.time_bin, p.threshold, p.rho, p.max_window, p.directions) == (64, 6.0, 1.5, 16, 'both')
    assert (p.level_iterations, p.level_clip, p.extend_freq, p.extend_time, p.extend_pols) \
        == (2, 4.0, 0.5, 0.5, True)
    assert p.mask(5).tolist() == [1] * 5
    assert p.factors().dtype == np.float64
    assert p.factors().tolist() == [6.0, 6.0 / 1.5, 6.0 / 1.5 ** 2, 6.0 / 1.5 ** 3, 6.0 / 1.5 ** 4]
    assert RFIFlagParameters(max_window=1).factors().tolist() == [6.0]
    assert len(RFIFlagParameters(max_window=32, rho=1.0).factors()) == 6
    assert RFIFlagParameters(line_ranges=[(2, 4)]).mask(6).tolist() == [1, 1, 0, 0, 1, 1]
    assert RFIFlagParameters(fit_mask=[1, 0, 2]).mask(3).tolist() == [1, 0, 1]
    with pytest.raises(ValueError):
        RFIFlagParameters(fit_mask=[1, 0, 2]).mask(4)
    with pytest.raises(ValueError):
        RFIFlagParameters(line_ranges=[(2, 9)]).mask(6)
    assert 'line_ranges=[(2, 4)]' in repr(RFIFlagParameters(line_ranges=[(2, 4)]))


@pytest.mark.parametrize('kwargs', [
    dict(time_bin=0), dict(time_bin=65), dict(time_bin=2.5), dict(time_bin='x'),
    dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=np.nan), dict(threshold=np.inf),
    dict(threshold='high'), dict(rho=0.9), dict(rho=np.nan), dict(rho=np.inf),
    dict(max_window=0), dict(max_window=3), dict(max_window=64), dict(max_window=12),
    dict(directions='all'), dict(directions=None),
    dict(level_iterations=-1), dict(level_iterations=5), dict(level_iterations=1.5),
    dict(level_clip=0.0), dict(level_clip=np.nan),
    dict(extend_freq=0.0), dict(extend_freq=1.5), dict(extend_freq=np.nan), dict(extend_freq=True),
    dict(extend_time=0.0), dict(extend_time=-0.5), dict(extend_time=np.nan),
    dict(extend_pols=1), dict(extend_pols=None),
    dict(fit_mask=[1, 1], line_ranges=[(0, 1)]), dict(fit_mask=[0, 0]), dict(fit_mask=[[1]]),
    dict(line_ranges=[(3, 2)]), dict(line_ranges=[(-1, 2)]),
])
def test_parameters_refuse(kwargs):
    with pytest.raises(ValueError):
        RFIFlagParameters(**kwargs)


# ---- hand-made planes -------------------------------------------------------------------------------
def test_a_single_spike_is_caught_by_the_window_of_one_and_by_nothing_else():
    vis, weights, ids = cases.ones(16, 16)
    cases.put(vis, weights, 5, 3, 0, 100.0)
    for max_window in (1, 2, 16, 32):
        flags, level, counts = _run(vis, weights, ids, RFIFlagParameters(16, max_window=max_window))
        assert _only(flags, [(5, 3, 0)]) and counts == (255, 1, 0)
        assert level.tolist() == [[1.0]]                        # the spike is clipped out of it
    # one sample of 6 (5 above the level) is nothing to any window
    cases.put(vis, weights, 5, 3, 0, 6.0)
    flags, level, counts = _run(vis, weights, ids, RFIFlagParameters(16))
    assert not flags.any() and counts == (256, 0, 0)


@pytest.mark.parametrize('direction', ['freq', 'time'])
def test_a_run_of_four_is_caught_by_the_window_of_four(direction):
    vis, weights, ids = cases.ones(16, 16)
    run = [(c, 3, 0) for c in range(6, 10)] if direction == 'freq' else [(5, r, 0) for r in range(6, 10)]
    for at in run:
        cases.put(vis, weights, *at, 4.0)
    for directions in (direction, 'both'):
        flags, level, counts = _run(vis, weights, ids, RFIFlagParameters(16, directions=directions))
        assert _only(flags, run) and counts == (252, 4, 0)
        # a sample of the run is below 6 and 4 levels, above 2.67 of them; three and an ordinary one
        # are not above 4 x 2.67
        L = level[0, 0]
        assert 4.0 * L > 4.0 - L > 6.0 / 2.25 * L > (3.0 * (4.0 - L) + (1.0 - L)) / 4.0
    flags, _, _ = _run(vis, weights, ids, RFIFlagParameters(16, max_window=2))
    assert not flags.any()
    other = 'time' if direction == 'freq' else 'freq'
    flags, _, _ = _run(vis, weights, ids, RFIFlagParameters(16, directions=other))
    assert not flags.any()


def test_a_protected_sample_inside_a_window_counts_as_the_threshold_and_stays():
    vis, weights, ids = cases.ones(16, 16)
    run = [(4, 3, 0), (5, 3, 0), (7, 3, 0), (8, 3, 0)]
    for at in run:
        cases.put(vis, weights, *at, 4.0)
    vis[6] = 100.0                                              # the line, bright and constant
    params = RFIFlagParameters(16, line_ranges=[(6, 7)])
    flags, level, counts = _run(vis, weights, ids, params)
    assert _only(flags, run) and counts == (252, 4, 0)
    # with the channel searched, the line is all the flagger sees
    flags, level, counts = _run(vis, weights, ids, RFIFlagParameters(16))
    assert flags[6].all()


def test_a_bright_constant_protected_channel_is_never_flagged_without_extend_freq():
    vis, weights, ids = cases.ones(16, 16, P=2)
    vis[6:8] = 100.0
    hits = [(c, 3, 0) for c in (0, 1, 2, 3, 4, 5, 8, 9, 10, 11)]
    for at in hits:
        cases.put(vis, weights, *at, 100.0)
    params = RFIFlagParameters(16, line_ranges=[(6, 8)], extend_freq=None)
    flags, _, _ = _run(vis, weights, ids, params)
    assert not flags[6:8].any() and flags[:, 3, 0].sum() == 10


def test_a_row_hit_in_more_than_half_its_channels_is_flagged_whole():
    for hit, whole in ((8, True), (7, False)):                  # of 14 mask channels
        vis, weights, ids = cases.ones(16, 16)
        vis[6:8] = 100.0
        chosen = [0, 2, 4, 8, 10, 12, 14, 15][:hit]
        for c in chosen:
            cases.put(vis, weights, c, 3, 0, 100.0)
        flags, level, counts = _run(vis, weights, ids, RFIFlagParameters(16, line_ranges=[(6, 8)]))
        assert level.tolist() == [[1.0]]
        want = [(c, 3, 0) for c in (range(16) if whole else chosen)]
        assert _only(flags, want)
        assert counts == (256 - len(want), len(want), 0)


def test_a_channel_hit_in_more_than_half_its_rows_is_flagged_for_the_group():
    for hit, whole in ((5, True), (4, False)):                  # of 8 rows
        vis, weights, ids = cases.ones(16, 8, groups=2)
        chosen = [0, 2, 4, 6, 7][:hit]
        for r in chosen:
            cases.put(vis, weights, 2, 8 + r, 0, 100.0)
        flags, level, counts = _run(vis, weights, ids, RFIFlagParameters(8))
        want = [(2, 8 + r, 0) for r in (range(8) if whole else chosen)]
        assert _only(flags, want) and counts[1:] == (len(want), 0)


def test_extend_pols_on_and_off():
    vis, weights, ids = cases.ones(16, 16, P=3)
    cases.put(vis, weights, 5, 3, 1, 100.0)
    weights[5, 3, 2] = 0.0                                      # not usable: never flagged
    flags, _, counts = _run(vis, weights, ids, RFIFlagParameters(16))
    assert _only(flags, [(5, 3, 0), (5, 3, 1)]) and counts == (3 * 256 - 3, 2, 0)
    flags, _, counts = _run(vis, weights, ids, RFIFlagParameters(16, extend_pols=False))
    assert _only(flags, [(5, 3, 1)]) and counts == (3 * 256 - 2, 1, 0)


def test_a_group_without_weight_is_skipped_and_left_alone():
    vis, weights, ids = cases.ones(8, 4, P=2, groups=3)
    weights[:, 4:8, 1] = 0.0
    weights[:, 8:12, 0] = -2.0
    vis[3, 9, 0] = np.nan
    cases.put(vis, weights, 2, 5, 0, 100.0)
    flags, level, counts = _run(vis, weights, ids, RFIFlagParameters(4))
    # (the spike's other polarization has no level, so extend_pols has nothing to flag there)
    assert _only(flags, [(2, 5, 0)]) and counts == (4 * 32 - 1, 1, 2)
    assert np.isnan(level).tolist() == [[False, False], [False, True], [True, False]]
    # a level that is not above 0: visibilities of 0
    vis[:, 0:4, 0] = 0.0
    _, level, counts = _run(vis, weights, ids, RFIFlagParameters(4))
    assert np.isnan(level[0, 0]) and counts[2] == 3


def test_no_window_crosses_a_group_boundary_or_the_end_of_the_band():
    # the run of four lies across two groups: no window of four has it, windows of two do not mind it
    vis, weights, ids = cases.ones(16, 8, groups=2)
    for r in (6, 7, 8, 9):
        cases.put(vis, weights, 5, r, 0, 4.0)
    flags, _, _ = _run(vis, weights, ids, RFIFlagParameters(8, directions='time'))
    assert not flags.any()
    # the same rows as ONE group are flagged
    flags, _, _ = _run(vis, weights, np.zeros(16, np.int32), RFIFlagParameters(16, directions='time'))
    assert _only(flags, [(5, r, 0) for r in (6, 7, 8, 9)])
    # a run that ends with the band is seen by the last window and by no window past it
    vis, weights, ids = cases.ones(16, 16)
    for c in (12, 13, 14, 15):
        cases.put(vis, weights, c, 2, 0, 4.0)
    flags, _, _ = _run(vis, weights, ids, RFIFlagParameters(16, directions='freq'))
    assert _only(flags, [(c, 2, 0) for c in (12, 13, 14, 15)])
    # windows longer than the band or the group do not exist
    vis, weights, ids = cases.ones(3, 3)
    cases.put(vis, weights, 1, 1, 0, 5.0)
    flags, _, _ = _run(vis, weights, ids, RFIFlagParameters(3, max_window=32))
    assert not flags.any()


@pytest.mark.parametrize('seed', range(6))
def test_twin_against_the_loops_on_noisy_blocks(seed):
    """The blocks the device is run on, small: every embedded feature, every direction."""
    rng = np.random.default_rng(seed)
    C, N, P = [(7, 40, 2), (17, 30, 1), (1, 50, 3), (5, 64, 4), (33, 12, 2), (2, 70, 1)][seed]
    vis, weights, ids, mask = cases.inputs(C, N, P, seed)
    flagged = 0
    for directions in cases.DIRECTIONS:
        params = RFIFlagParameters(int(rng.choice([1, 3, 16, 64])), max_window=int(rng.choice([1, 2, 8, 32])),
                                   directions=directions, level_iterations=int(rng.integers(5)),
                                   fit_mask=mask, extend_pols=bool(seed % 2))
        flags, _, counts = _run(vis, weights, ids, params)
        flagged += counts[1]
    assert flagged > 0


@pytest.mark.parametrize('make', [bands.straddle, bands.alternate_words, bands.word0_empty])
def test_twin_against_the_loops_past_one_mask_word(make):
    """97 channels, four words of the device's mask, windows of up to 32 in both directions, on a
    block small enough for the loops: the twin the device is compared with."""
    C, N, P = 97, 10, 2
    vis, weights, ids, mask = cases.band_inputs(C, N, P, 97, make(C))
    ids = np.repeat(np.array([3, 1], np.int32), 5)
    params = RFIFlagParameters(4, max_window=32, directions='both', fit_mask=mask)
    flags, level, counts = _run(vis, weights, ids, params)
    assert counts[0] > 0 and counts[1] > 0


@pytest.mark.parametrize('C', [97, 1025])
def test_long_band_cases_hold_what_they_were_made_for(C):
    """The blocks of test_rfiflag_gpu.test_device_against_twin_past_one_mask_word, with the twin
    alone: every plane's blocks together have samples kept, samples flagged and pairs skipped; the
    bright channel at 32 is protected and never flagged, the searched samples of the hot run are
    flagged, and (looked at in the band of 97) the windows of 32 flag what the shorter ones leave."""
    longest = False
    for N, P in bands.PLANES:
        total = np.zeros(3, np.int64)
        for i, (name, mask) in enumerate(bands.masks(C)):
            time_bin = cases.TIME_BINS[i % 3]
            vis, weights, ids, mask = cases.band_inputs(C, N, P, 100 * C + 10 * N + i, mask)
            assert not mask[cases.BRIGHT] and mask.any()
            params = RFIFlagParameters(time_bin, max_window=32, directions='both',
                                       level_iterations=cases.LEVEL_ITERATIONS[i % 3], fit_mask=mask,
                                       extend_pols=bool(i % 2))
            _, flags, level, counts = rfiflag_host(vis, weights, ids, params)
            total += counts
            run = slice(*cases.HOT)
            searched = mask[run].astype(bool)
            if searched.any():
                assert flags[run, cases.hot_row(ids), 0][searched].all(), (C, N, P, name)
            if C == 97:
                shorter = RFIFlagParameters(time_bin, max_window=16, directions='both',
                                            level_iterations=cases.LEVEL_ITERATIONS[i % 3], fit_mask=mask,
                                            extend_pols=bool(i % 2))
                longest |= not np.array_equal(rfiflag_host(vis, weights, ids, shorter)[1], flags)
        assert total.min() > 0
    assert longest or C != 97


# ---- pure noise -------------------------------------------------------------------------------------
def _noise(seed=1):
    rng = np.random.default_rng(seed)
    C, N = 64, 4096
    vis = (rng.normal(size=(C, N, 1)) + 1j * rng.normal(size=(C, N, 1))).astype(np.complex64)
    return vis, np.ones((C, N, 1), np.float32), np.repeat(np.arange(N // 64, dtype=np.int32), 64)


def test_defaults_on_pure_noise():
    """Gaussian noise under equal weights, 64 channels x 4096 rows in groups of 16, the defaults:
    the twin flags 0.0054 of the samples (seed 1: 1415 of 262144; 0.0019 by the windows of one
    sample alone, 0.0053 before the extensions).  z / mean is exponentially distributed and the
    clipped level is 0.90 of the mean, so a single sample passes 7 levels with probability
    exp(-6.3) = 0.0018; the longer windows add the rest.  The cap that keeps the defaults from eating
    data is twice the measured value."""
    vis, weights, ids = _noise()
    _, flags, level, counts = rfiflag_host(vis, weights, ids, RFIFlagParameters(time_bin=16))
    fraction = counts[1] / (counts[0] + counts[1])
    print('flagged fraction of pure noise under the defaults: {:.4f}'.format(fraction))
    assert counts[2] == 0 and counts[0] + counts[1] == flags.size
    assert 0.88 < np.mean(level) / 2.0 < 0.92
    assert 0.0 < fraction < 2 * 0.0054


# ---- the twin's own checks --------------------------------------------------------------------------
def test_twin_refuses_what_it_cannot_take():
    vis, weights, ids = cases.ones(4, 4)
    params = RFIFlagParameters(4)
    with pytest.raises(TypeError):
        rfiflag_host(vis.astype(np.complex128), weights, ids, params)
    with pytest.raises(TypeError):
        rfiflag_host(vis, weights.astype(np.float64), ids, params)
    with pytest.raises(ValueError):
        rfiflag_host(vis, weights[:3], ids, params)
    with pytest.raises(ValueError):
        rfiflag_host(vis, weights, ids[:3], params)
    with pytest.raises(ValueError):
        rfiflag_host(vis, weights, ids, RFIFlagParameters(4, fit_mask=[1] * 5))
    new, flags, level, counts = rfiflag_host(vis[:, :0], weights[:, :0], ids[:0], params)
    assert new.shape == flags.shape == (4, 0, 1) and level.shape == (0, 1) and counts == (0, 0, 0)


# ---- the C entry point, without a device ------------------------------------------------------------
def test_entry_point_refuses_before_any_hip_call():
    from katsdpimager_amd import _lib
    fn = _lib.lib().kimg_rfi_flag
    # host addresses: nothing dereferences them
    ptr = dict(vis=0x10000000, weights=0x20000000, offsets=0x30000000, row_group=0x40000000,
               flags=0x50000000, level=0x58000000, workspace=0x60000000, counts=0x70000000)
    full = np.ones(16, np.uint8)
    five = np.array([6.0, 4.0, 3.0, 2.0, 1.5])
    enough = 9 * 16 * 16 + 24 * 16

    def call(C=16, N=8, P=2, mask=full, vp=16, wp=16, G=2, time_bin=4, factors=five, max_window=16,
             directions=3, iterations=2, clip=4.0, ef=0.5, et=0.5, pols=1, bytes=enough, **pointers):
        p = {k: ctypes.c_void_p(v) for k, v in ptr.items()}
        p.update({k: (None if v is None else ctypes.c_void_p(v)) for k, v in pointers.items()})
        m = None if mask is None else mask.ctypes.data_as(ctypes.c_void_p)
        f = None if factors is None else factors.ctypes.data_as(ctypes.c_void_p)
        return fn(p['vis'], vp, p['weights'], wp, C, N, P, m, p['offsets'], G, p['row_group'], time_bin,
                  f, max_window, directions, iterations, clip, ef, et, pols, p['flags'], p['level'],
                  p['workspace'], bytes, p['counts'], None)
    assert call(N=0, vp=0, wp=0, G=0, bytes=0) == 0             # the checks pass; an empty plane
    for null in ptr:
        assert call(N=0, **{null: None}) == EINVAL
    assert call(N=0, mask=None) == EINVAL and call(N=0, factors=None) == EINVAL
    assert call(N=0, C=0) == EINVAL
    assert call(N=-1) == EINVAL
    for pols in (0, 5, -1):
        assert call(N=0, P=pols) == EINVAL
    for time_bin in (0, 65, -3):
        assert call(N=0, time_bin=time_bin) == EINVAL
    for max_window in (0, 3, 64, -2):
        assert call(N=0, max_window=max_window) == EINVAL
    for directions in (0, 4, -1):
        assert call(N=0, directions=directions) == EINVAL
    assert call(N=0, iterations=-1) == EINVAL and call(N=0, iterations=5) == EINVAL
    assert call(N=0, clip=0.0) == EINVAL and call(N=0, clip=np.nan) == EINVAL
    for share in (-0.5, 1.5, np.nan):
        assert call(N=0, ef=share) == EINVAL and call(N=0, et=share) == EINVAL
    assert call(N=0, ef=0.0, et=0.0, pols=0) == 0               # no extension at all
    assert call(N=0, factors=np.array([6.0, 4.0, 0.0, 2.0, 1.0])) == EINVAL
    assert call(N=0, factors=np.array([6.0, 4.0, np.nan, 2.0, 1.0])) == EINVAL
    assert call(N=0, factors=np.array([6.0, 4.0, 0.0]), max_window=2) == 0      # (two are read)
    assert call(vp=15) == EINVAL and call(wp=15) == EINVAL
    assert call(N=0, C=16385, mask=np.ones(16385, np.uint8)) == EUNSUPPORTED
    assert call(N=0, C=16384, mask=np.ones(16384, np.uint8)) == 0
    assert call(N=2 ** 31, vp=2 ** 33, wp=2 ** 33) == EUNSUPPORTED
    # the groups cannot be these rows': none, more than rows, too few for the bin
    assert call(G=0) == EINVAL and call(G=9) == EINVAL and call(G=1) == EINVAL
    assert call(bytes=enough - 1) == EWORKSPACE
    assert call(workspace=ptr['workspace'] + 4) == EINVAL


# ---- build and ABI surface --------------------------------------------------------------------------
def test_symbol_is_declared_exported_and_prototyped():
    from katsdpimager_amd import _lib, build, statwt
    assert 'rfiflag.hip' in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, 'rfiflag.hip'))
    assert 'kimg_rfi_flag' in _lib.PROTOTYPES and len(_lib.PROTOTYPES['kimg_rfi_flag'][1]) == 26
    assert _lib.lib().kimg_rfi_flag is not None
    header = open(os.path.join(os.path.dirname(build.HERE), 'include', 'kimg.h')).read()
    assert re.search(r'^int kimg_rfi_flag\(', header, re.M)
    defines = {k: int(v) for k, v in re.findall(r'^#define (KIMG_RFIFLAG_\w+) (\d+)$', header, re.M)}
    assert defines['KIMG_RFIFLAG_MAX_WINDOW'] == rfiflag.MAX_WINDOW == 32
    assert defines['KIMG_RFIFLAG_MAX_LEVEL_ITERATIONS'] == rfiflag.MAX_LEVEL_ITERATIONS == 4
    assert defines['KIMG_RFIFLAG_WORKSPACE_PER_ELEMENT'] == rfiflag.WORKSPACE_PER_ELEMENT
    assert defines['KIMG_RFIFLAG_WORKSPACE_PER_ROW'] == rfiflag.WORKSPACE_PER_ROW
    assert rfiflag.DIRECTIONS == {'time': defines['KIMG_RFIFLAG_TIME'], 'freq': defines['KIMG_RFIFLAG_FREQ'],
                                  'both': defines['KIMG_RFIFLAG_TIME'] | defines['KIMG_RFIFLAG_FREQ']}
    assert rfiflag.MAX_BIN == statwt.MAX_BIN
    assert rfiflag.RFIFlag.workspace_bytes(3, 5, 2) == 9 * 30 + 24 * 10
    assert _lib.lib().kimg_version() == _lib.VERSION == 5


# ---- the loader's keyword ---------------------------------------------------------------------------
class _Recorder:
    queue = None

    def __init__(self, num_channels):
        self.num_channels = num_channels
        self.calls = []

    def add(self, *args):
        self.calls.append(('add',) + args)

    def close(self):
        self.calls.append(('close',))


class _Dataset(loader.LoaderArrays):
    blocks_read = 0

    def data_iter(self, *args, **kwargs):
        for chunk in super().data_iter(*args, **kwargs):
            self.blocks_read += 1
            yield chunk


def _dataset(rows=50, C=6):
    rng = np.random.default_rng(2)
    vis = (rng.normal(size=(rows, C, 1)) + 1j * rng.normal(size=(rows, C, 1))).astype(np.complex64)
    return _Dataset(rng.normal(size=(rows, 3)).astype(np.float32), vis,
                    np.ones((rows, C, 1), np.float32), np.arange(rows) % 7,
                    1.4e9 + 1e6 * np.arange(C), [0])


def test_loader_without_the_keyword_takes_the_old_path():
    ident = np.identity(1, np.complex64)
    rec, dataset = _Recorder(6), _dataset()
    assert loader.preprocess_visibilities(dataset, rec, 0, 6, (ident, None), vis_load=6 * 20,
                                          rfiflag=None) is rec
    assert [call[0] for call in rec.calls] == ['add', 'add', 'add', 'close'] and dataset.blocks_read == 3
    assert isinstance(rec.calls[0][2], np.ndarray) and not hasattr(rec, 'rfiflag_counts')


def test_loader_refuses_a_mask_of_another_length_before_any_block_is_read():
    from katsdpimager_amd import spectral
    ident = np.identity(1, np.complex64)
    for kwargs in (dict(rfiflag=RFIFlagParameters(fit_mask=[1] * 5)),
                   dict(rfiflag=RFIFlagParameters(line_ranges=[(5, 7)])),
                   # the mask spans the spectral filter's outputs, three here
                   dict(rfiflag=RFIFlagParameters(fit_mask=[1] * 6),
                        spectral=spectral.SpectralParameters.average(2))):
        rec, dataset = _Recorder(3 if 'spectral' in kwargs else 6), _dataset()
        with pytest.raises(ValueError):
            loader.preprocess_visibilities(dataset, rec, 0, 6, (ident, None), **kwargs)
        assert not rec.calls and dataset.blocks_read == 0
