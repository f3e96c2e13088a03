"""Statistical reweighting without a device: the parameters object, the grouping, the numpy twin
(statwt.statwt_host, the executable form of the contract in include/kimg.h) against closed forms and
hand-made cases, the noise it promises, the argument checks of kimg_statwt (they run before any HIP
call), the ABI surface, and the loader's keyword; and, for test_statwt_gpu.py, that every block of
statwt_cases.py holds the groups it was made to hold."""
import ctypes
import os
import re

import numpy as np
import pytest

import band_cases as bands
import statwt_cases as cases
from katsdpimager_amd import loader, statwt
from katsdpimager_amd.statwt import StatWtParameters, group_offsets, statwt_host

EINVAL, EUNSUPPORTED, EWORKSPACE = -10001, -10002, -10003


def _noise(rng, C, N, P, sigma=1.0):
    return ((rng.normal(size=(C, N, P)) + 1j * rng.normal(size=(C, N, P))) * sigma).astype(np.complex64)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the parameters object --------------------------------------------------------------------------
def test_parameters_and_their_mask():
    p = StatWtParameters()
    assert (p.time_bin, p.min_samples, p.chi2_range) == (1, 8, (0.0, np.inf))
    assert p.mask(5).tolist() == [1] * 5 and p.mask(5).dtype == np.uint8
    p = StatWtParameters(8, line_ranges=[(2, 4)], min_samples=2, chi2_range=(0.5, 2))
    assert p.mask(6).tolist() == [1, 1, 0, 0, 1, 1] and p.chi2_range == (0.5, 2.0)
    with pytest.raises(ValueError):
        p.mask(3)                                   # a range beyond the band
    p = StatWtParameters(64, fit_mask=[1, 0, 2])
    assert p.mask(3).tolist() == [1, 0, 1]
    with pytest.raises(ValueError):
        p.mask(4)
    with pytest.raises(ValueError):
        StatWtParameters(line_ranges=[(0, 4)]).mask(4)      # nothing left
    assert 'time_bin' not in repr(p) and repr(p).startswith('StatWtParameters(64, fit_mask=')


@pytest.mark.parametrize('kwargs', [
    dict(time_bin=0), dict(time_bin=65), dict(time_bin=1.5), dict(time_bin='a'),
    dict(min_samples=1), dict(min_samples=2.5), dict(min_samples=None),
    dict(fit_mask=[1, 1], line_ranges=[(0, 1)]),
    dict(fit_mask=[[1, 1]]), dict(fit_mask=[]), dict(fit_mask=[0, 0]),
    dict(line_ranges=[(3, 2)]), dict(line_ranges=[(-1, 2)]),
    dict(chi2_range=(1.0,)), dict(chi2_range=(2.0, 1.0)), dict(chi2_range=(1.0, 1.0)),
    dict(chi2_range=(-1.0, 1.0)), dict(chi2_range=(np.nan, 1.0)), dict(chi2_range=(0.0, np.nan)),
    dict(chi2_range='ab'),
])
def test_parameters_refuse(kwargs):
    with pytest.raises(ValueError):
        StatWtParameters(**kwargs)


# ---- grouping ---------------------------------------------------------------------------------------
def test_group_offsets():
    assert group_offsets(np.zeros(0, int), 4).tolist() == [0]
    assert group_offsets([7], 4).tolist() == [0, 1]
    # runs of length 1, time_bin, time_bin + 1, and ids that return later in the block (a new run)
    ids = [5] + [3] * 4 + [5] * 5 + [3] + [9] * 9
    got = group_offsets(ids, 4)
    assert got.dtype == np.int32
    assert got.tolist() == [0, 1, 5, 9, 10, 11, 15, 19, 20]
    assert group_offsets(ids, 1).tolist() == list(range(21))
    assert group_offsets(ids, 64).tolist() == [0, 1, 5, 10, 11, 20]
    assert group_offsets(np.array(ids, np.uint8), 3).tolist() == [0, 1, 4, 5, 8, 10, 11, 14, 17, 20]
    rng = np.random.default_rng(0)
    for time_bin in (1, 3, 64):
        ids = cases.baselines(rng, 1000)
        g = group_offsets(ids, time_bin)
        assert g[0] == 0 and g[-1] == 1000 and (np.diff(g) >= 1).all() and (np.diff(g) <= time_bin).all()
        for a, b in zip(g[:-1], g[1:]):
            assert (ids[a:b] == ids[a]).all()
        # a boundary is a change of id or a whole bin since the run began
        for a in g[1:-1]:
            if ids[a] == ids[a - 1]:
                start = a
                while start > 0 and ids[start - 1] == ids[a]:
                    start -= 1
                assert (a - start) % time_bin == 0
    with pytest.raises(ValueError):
        group_offsets(np.zeros((2, 2), int), 4)
    with pytest.raises(ValueError):
        group_offsets([1, 2], 0)
    with pytest.raises(ValueError):
        group_offsets([1, 2], 65)


# ---- the twin against closed forms ------------------------------------------------------------------
def test_equal_weights_give_one_over_the_sample_variance():
    rng = np.random.default_rng(1)
    C, rows, P, time_bin = 12, 20, 2, 5
    vis = _noise(rng, C, rows, P, 2.5)
    ids = np.repeat([4, 9], 10)
    params = StatWtParameters(time_bin, line_ranges=[(3, 5)])
    fit = params.mask(C).astype(bool)
    for w in (1.0, 0.3):
        weights = np.full((C, rows, P), w, np.float32)
        new, chi2, counts = statwt_host(vis, weights, ids, params)
        assert new.dtype == np.float32 and chi2.shape == (4, P) and counts == (4 * P, 0)
        for g in range(4):
            for p in range(P):
                v = vis[fit, g * 5:(g + 1) * 5, p].astype(np.complex128).ravel()
                resid = np.concatenate((v.real - v.real.mean(), v.imag - v.imag.mean()))
                # chi2 = w sum |v - mean|^2 / (2 (M - 1)): the residuals have 2 M entries, ddof 2
                want = 1.0 / np.var(resid, ddof=2)
                assert abs(float(np.float32(w)) / chi2[g, p] / want - 1.0) <= 1e-12
                # every channel of the group's rows, line channels included, rounded once
                np.testing.assert_array_equal(new[:, g * 5:(g + 1) * 5, p], np.float32(np.float32(w) / chi2[g, p]))


def test_scale_of_the_input_weights_does_not_matter():
    rng = np.random.default_rng(2)
    C, rows, P = 10, 24, 3
    vis = _noise(rng, C, rows, P)
    weights = rng.uniform(0.5, 2.0, (C, rows, P)).astype(np.float32)
    ids = np.repeat(np.arange(3), 8)
    params = StatWtParameters(4)
    base, chi2, _ = statwt_host(vis, weights, ids, params)
    for k in (3.0, 1e-3, 7e5):
        scaled, chi2_k, _ = statwt_host(vis, (weights * np.float32(k)).astype(np.float32), ids, params)
        # (the scaled weights are rounded to float32 once more on the way in, and the result once)
        assert np.abs(scaled / base - 1.0).max() <= 2.0 ** -22
        np.testing.assert_allclose(chi2_k, k * chi2, rtol=2.0 ** -22)
    # relative channel weights survive
    ratio = base / weights
    assert np.abs(ratio / ratio[0] - 1.0).max() <= 2.0 ** -22


def test_a_constant_offset_leaves_chi2_alone():
    """What the two-pass form is for: continuum 100 times the noise.  The noise is made of multiples
    of 2^-12 so that adding the offset is exact in float32 and the inputs differ by the offset alone."""
    rng = np.random.default_rng(3)
    C, rows, P = 16, 12, 1
    noise = np.round(rng.normal(size=(C, rows, P, 2)) * 4096.0) / 4096.0
    ids = np.repeat([1, 2], 6)
    params = StatWtParameters(6)
    weights = rng.uniform(0.5, 2.0, (C, rows, P)).astype(np.float32)
    plain = (noise[..., 0] + 1j * noise[..., 1]).astype(np.complex64)
    offset = ((noise[..., 0] + 100.0) + 1j * (noise[..., 1] - 100.0)).astype(np.complex64)
    assert np.array_equal(offset.real.astype(np.float64) - 100.0, noise[..., 0])
    _, chi2, counts = statwt_host(plain, weights, ids, params)
    _, chi2_offset, _ = statwt_host(offset, weights, ids, params)
    assert counts == (2, 0)
    assert np.abs(chi2_offset / chi2 - 1.0).max() <= 1e-9
    # a one-pass sum of squares in float32-sized steps would not: the data really are 100 sigma off
    assert np.abs(offset).min() > 90


def test_noise_of_every_baseline_is_what_its_new_weight_says():
    """40 baselines with sigma in [0.5, 4], weights 1, 64 fit channels, time_bin 8: M = 512, chi2
    has relative standard deviation 1 / sqrt(M - 1) = 0.044 (a chi-square of 2 (M - 1) degrees of
    freedom), and every group's w' sigma^2 lies within 1 +- 5 * 0.044."""
    rng = np.random.default_rng(2025)
    baselines, times, C = 40, 16, 64
    sigma = rng.uniform(0.5, 4.0, baselines)
    ids = np.repeat(np.arange(baselines), times)
    vis = _noise(rng, C, baselines * times, 1) * np.repeat(sigma, times)[None, :, None].astype(np.float32)
    new, chi2, counts = statwt_host(vis.astype(np.complex64), np.ones(vis.shape, np.float32), ids,
                                    StatWtParameters(8))
    assert counts == (80, 0)
    product = new[0, :, 0].astype(np.float64) * np.repeat(sigma, times) ** 2
    print('w\' sigma^2 between {:.4f} and {:.4f}'.format(product.min(), product.max()))
    assert np.abs(product - 1.0).max() <= 5 * 0.044


# ---- hand-made cases --------------------------------------------------------------------------------
def _one_group(rng, C=6, rows=2):
    return (_noise(rng, C, rows, 1), rng.uniform(0.5, 2.0, (C, rows, 1)).astype(np.float32),
            np.zeros(rows, np.int32))


def test_min_samples_is_met_exactly_or_not():
    rng = np.random.default_rng(5)
    vis, weights, ids = _one_group(rng)             # 12 samples
    weights[0, 0, 0] = 0.0
    weights[1, 0, 0] = -2.0
    vis[2, 1, 0] = complex(np.nan, 0.0)
    vis[3, 1, 0] = complex(0.0, np.inf)             # 8 left
    new, chi2, counts = statwt_host(vis, weights, ids, StatWtParameters(2, min_samples=8))
    assert counts == (1, 0) and chi2[0, 0] > 0
    # the four unusable samples are dropped from the statistic ...
    usable = (weights > 0) & np.isfinite(vis.real) & np.isfinite(vis.imag)
    w = weights[usable].astype(np.float64)
    v = vis[usable].astype(np.complex128)
    mean = (w * v).sum() / w.sum()
    np.testing.assert_allclose(chi2[0, 0], (w * np.abs(v - mean) ** 2).sum() / (2 * 7), rtol=1e-13)
    # ... their weights are rescaled where positive and untouched, bit for bit, where not
    assert new[2, 1, 0] == np.float32(np.float64(weights[2, 1, 0]) / chi2[0, 0])
    assert new[0, 0, 0] == 0 and not np.signbit(new[0, 0, 0])
    assert _bits(new[1, 0, 0]) == _bits(np.float32(-2.0))
    # one sample fewer: flagged, every weight +0
    weights[4, 0, 0] = 0.0
    new, chi2, counts = statwt_host(vis, weights, ids, StatWtParameters(2, min_samples=8))
    assert counts == (0, 1) and not _bits(new).any() and chi2[0, 0] > 0
    assert statwt_host(vis, weights, ids, StatWtParameters(2, min_samples=7))[2] == (1, 0)


def test_groups_without_weight_or_without_scatter_are_flagged():
    rng = np.random.default_rng(6)
    vis, weights, ids = _one_group(rng)
    new, chi2, counts = statwt_host(vis, np.zeros_like(weights), ids, StatWtParameters(2, min_samples=2))
    assert counts == (0, 1) and np.isnan(chi2[0, 0]) and not _bits(new).any()
    constant = np.full_like(vis, complex(1.5, -0.5))
    new, chi2, counts = statwt_host(constant, np.ones_like(weights), ids, StatWtParameters(2, min_samples=2))
    assert counts == (0, 1) and chi2[0, 0] == 0.0 and not _bits(new).any()
    # a single usable sample: chi2 is NaN, not 0 / 0 by accident
    weights[:] = 0.0
    weights[1, 1, 0] = 1.0
    new, chi2, counts = statwt_host(vis, weights, ids, StatWtParameters(2, min_samples=2))
    assert counts == (0, 1) and np.isnan(chi2[0, 0]) and not _bits(new).any()
    # an infinite weight is not usable, and is rescaled like any positive weight
    vis, weights, ids = _one_group(rng)
    reference = statwt_host(vis[1:], weights[1:], ids, StatWtParameters(2))
    weights[0, :, 0] = np.inf
    new, chi2, counts = statwt_host(vis, weights, ids, StatWtParameters(2))
    assert chi2[0, 0] == reference[1][0, 0] and np.isinf(new[0]).all()
    assert np.array_equal(_bits(new[1:]), _bits(reference[0]))


def test_a_nan_in_a_line_channel_has_no_effect():
    rng = np.random.default_rng(7)
    vis, weights, ids = _one_group(rng, C=8, rows=3)
    params = StatWtParameters(3, line_ranges=[(2, 4)])
    want = statwt_host(vis, weights, ids, params)
    vis[2, 1, 0] = complex(np.nan, np.nan)
    vis[3, 0, 0] = complex(np.inf, 1.0)
    got = statwt_host(vis, weights, ids, params)
    assert got[2] == want[2] == (1, 0)
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and got[1][0, 0] == want[1][0, 0]
    # the line channels' weights are rescaled like the others
    assert (got[0][2:4] != weights[2:4]).all()


def test_both_sides_of_the_chi2_range():
    rng = np.random.default_rng(8)
    C, P = 32, 1
    ids = np.repeat(np.arange(3), 4)
    scale = np.repeat([0.1, 1.0, 10.0], 4)[None, :, None].astype(np.float32)
    vis = (_noise(rng, C, 12, P) * scale).astype(np.complex64)
    weights = np.ones((C, 12, P), np.float32)
    _, chi2, counts = statwt_host(vis, weights, ids, StatWtParameters(4))
    assert counts == (3, 0) and chi2[0, 0] < 0.02 < 0.5 < chi2[1, 0] < 2 < 50 < chi2[2, 0]
    new, chi2_cut, counts = statwt_host(vis, weights, ids, StatWtParameters(4, chi2_range=(0.5, 2.0)))
    assert counts == (1, 2) and np.array_equal(chi2_cut, chi2)
    assert not _bits(new[:, :4]).any() and not _bits(new[:, 8:]).any() and (new[:, 4:8] > 0).all()
    # the ends are excluded
    edge = statwt_host(vis, weights, ids, StatWtParameters(4, chi2_range=(float(chi2[1, 0]), 1e9)))
    assert edge[2] == (1, 2) and not _bits(edge[0][:, :8]).any()
    edge = statwt_host(vis, weights, ids, StatWtParameters(4, chi2_range=(0.0, float(chi2[1, 0]))))
    assert edge[2] == (1, 2) and not _bits(edge[0][:, 4:]).any()


def test_twin_refuses_what_it_cannot_take():
    rng = np.random.default_rng(9)
    vis, weights, ids = _one_group(rng)
    with pytest.raises(TypeError):
        statwt_host(vis.astype(np.complex128), weights, ids, StatWtParameters())
    with pytest.raises(ValueError):
        statwt_host(vis, weights[:3], ids, StatWtParameters())
    with pytest.raises(ValueError):
        statwt_host(vis, weights, ids[:1], StatWtParameters())
    with pytest.raises(ValueError):
        statwt_host(vis, weights, ids, StatWtParameters(fit_mask=[1] * 5))


# ---- the blocks of test_statwt_gpu.py hold what they were made for -----------------------------------
@pytest.mark.parametrize('shape', range(len(cases.SHAPES)))
def test_device_cases_hold_their_hand_made_groups(shape):
    C, mask = cases.SHAPES[shape]
    seen = set()
    for N in cases.ROWS:
        for P in (1, 4):
            for time_bin in cases.TIME_BINS:
                vis, weights, ids, params, marks = cases.inputs(C, mask, N, P, time_bin,
                                                                1000 * shape + 10 * N + P)
                _, offsets, _, most = cases.parameters(C, mask, time_bin, ids)
                new, chi2, counts = statwt_host(vis, weights, ids, params)
                cases.assert_marks(marks, new, chi2, counts, weights, offsets, most, N, P)
                seen |= set(marks)
                if N == 1000 and most >= 8 and time_bin == 3:
                    assert {'low', 'high'} <= set(marks)
    assert {'empty', 'constant', 'samples'} <= seen
    assert ('exact' in seen) and ('low' in seen or C == 1)


@pytest.mark.parametrize('C', bands.CHANNELS)
def test_long_band_cases_hold_their_hand_made_groups(C):
    """The blocks of test_statwt_gpu.test_device_against_twin_past_one_mask_word, with the twin alone."""
    seen = set()
    turn = 0
    for i, (name, mask) in enumerate(bands.masks(C)):
        for N, P in bands.PLANES:
            time_bin = cases.TIME_BINS[turn % 3]
            turn += 1
            vis, weights, ids, params, marks = cases.inputs(C, mask, N, P, time_bin, 9000 * i + 10 * N + P + C)
            _, offsets, _, most = cases.parameters(C, mask, time_bin, ids)
            new, chi2, counts = statwt_host(vis, weights, ids, params)
            cases.assert_marks(marks, new, chi2, counts, weights, offsets, most, N, P)
            seen |= set(marks)
    assert {'exact', 'empty', 'constant'} <= seen


def _per_sample(vis, weights, ids, params):
    """The contract of kimg_statwt once more, one sample at a time in Python floats: (weights, chi2,
    counts).  It shares no line with the vectorised twin.  For small blocks."""
    C, N, P = vis.shape
    mask = params.mask(C)
    offsets = group_offsets(ids, params.time_bin)
    G = len(offsets) - 1
    lo, hi = params.chi2_range
    new = weights.copy()
    chi2 = np.full((G, P), np.nan)
    kept_groups = 0
    for g in range(G):
        rows = range(offsets[g], offsets[g + 1])
        for p in range(P):
            def usable(c, r):
                w, v = float(weights[c, r, p]), vis[c, r, p]
                return mask[c] and w > 0 and np.isfinite(w) and np.isfinite(v.real) and np.isfinite(v.imag)
            S0 = SR = SI = 0.0
            M = 0
            for r in rows:
                s0 = sr = si = 0.0
                for c in range(C):
                    if usable(c, r):
                        w = float(weights[c, r, p])
                        s0 += w
                        sr += w * float(vis[c, r, p].real)
                        si += w * float(vis[c, r, p].imag)
                        M += 1
                S0, SR, SI = S0 + s0, SR + sr, SI + si
            Q = 0.0
            if S0 > 0:
                mur, mui = SR / S0, SI / S0
                for r in rows:
                    q = 0.0
                    for c in range(C):
                        if usable(c, r):
                            dr = float(vis[c, r, p].real) - mur
                            di = float(vis[c, r, p].imag) - mui
                            t = dr * dr
                            t = t + di * di
                            q += float(weights[c, r, p]) * t
                    Q += q
            value = Q / (2.0 * (M - 1)) if M >= 2 else np.nan
            chi2[g, p] = value
            kept = M >= params.min_samples and lo < value < hi
            kept_groups += kept
            for r in rows:
                for c in range(C):
                    if not kept:
                        new[c, r, p] = 0.0
                    elif weights[c, r, p] > 0:
                        with np.errstate(over='ignore'):
                            new[c, r, p] = np.float32(float(weights[c, r, p]) / value)
    return new, chi2, (kept_groups, G * P - kept_groups)


@pytest.mark.parametrize('make', [bands.straddle, bands.word0_empty])
@pytest.mark.parametrize('time_bin', [1, 3])
def test_twin_against_the_per_sample_restatement_past_one_mask_word(make, time_bin):
    """65 channels, three words of the device's mask: the twin the device is compared with, bit for
    bit against the loops."""
    C, N, P = 65, 40, 2
    mask = make(C)
    vis, weights, ids, params, marks = cases.inputs(C, mask, N, P, time_bin, 65 + time_bin)
    got = statwt_host(vis, weights, ids, params)
    want = _per_sample(vis, weights, ids, params)
    assert np.array_equal(_bits(got[0]), _bits(want[0]))
    nan = np.isnan(want[1])
    assert np.array_equal(np.isnan(got[1]), nan)
    assert np.array_equal(got[1][~nan].view(np.uint64), want[1][~nan].view(np.uint64))
    assert got[2] == want[2] and got[2][0] >= 1 and got[2][1] >= 1


# ---- the C entry point, without a device ------------------------------------------------------------
def test_entry_point_refuses_before_any_hip_call():
    from katsdpimager_amd import _lib
    fn = _lib.lib().kimg_statwt
    # host addresses: nothing dereferences them
    ptr = dict(vis=0x10000000, weights=0x20000000, offsets=0x30000000, row_group=0x40000000,
               chi2=0x50000000, workspace=0x60000000, counts=0x70000000)
    full = np.ones(16, np.uint8)

    def call(C=16, N=8, P=2, mask=full, vp=16, wp=16, G=2, time_bin=4, min_samples=8, lo=0.0, hi=np.inf,
             bytes=36 * 16, **pointers):
        p = {k: ctypes.c_void_p(v) for k, v in ptr.items()}
        p.update({k: (None if v is None else ctypes.c_void_p(v)) for k, v in pointers.items()})
        m = None if mask is None else mask.ctypes.data_as(ctypes.c_void_p)
        return fn(p['vis'], vp, p['weights'], wp, C, N, P, m, p['offsets'], G, p['row_group'], time_bin,
                  min_samples, lo, hi, p['chi2'], p['workspace'], bytes, p['counts'], None)
    assert call(N=0, vp=0, wp=0, G=0, bytes=0) == 0         # the checks pass; an empty plane
    for null in ('vis', 'weights', 'offsets', 'row_group', 'workspace', 'counts'):
        assert call(N=0, **{null: None}) == EINVAL
    assert call(N=0, mask=None) == EINVAL
    assert call(N=0, chi2=None) == 0                        # chi2 is optional
    assert call(N=0, C=0) == EINVAL
    assert call(N=-1) == EINVAL
    for pols in (0, 5, -1):
        assert call(N=0, P=pols) == EINVAL
    for time_bin in (0, 65, -3):
        assert call(N=0, time_bin=time_bin) == EINVAL
    for min_samples in (1, 0, -8):
        assert call(N=0, min_samples=min_samples) == EINVAL
    assert call(N=0, lo=np.nan) == EINVAL and call(N=0, hi=np.nan) == EINVAL
    assert call(vp=15) == EINVAL and call(wp=15) == EINVAL
    assert call(N=0, C=16385, mask=np.ones(16385, np.uint8)) == EUNSUPPORTED
    assert call(N=0, C=16384, mask=np.ones(16384, np.uint8)) == 0
    assert call(N=2 ** 31, vp=2 ** 33, wp=2 ** 33) == EUNSUPPORTED
    # the groups cannot be these rows': none, more than rows, too few for the bin
    assert call(G=0) == EINVAL and call(G=9) == EINVAL and call(G=1) == EINVAL
    assert call(bytes=36 * 16 - 1) == EWORKSPACE
    assert call(workspace=ptr['workspace'] + 4) == EINVAL


# ---- build and ABI surface --------------------------------------------------------------------------
def test_symbol_is_declared_exported_and_prototyped():
    from katsdpimager_amd import _lib, build
    assert 'statwt.hip' in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, 'statwt.hip'))
    assert 'kimg_statwt' in _lib.PROTOTYPES and len(_lib.PROTOTYPES['kimg_statwt'][1]) == 20
    assert _lib.lib().kimg_statwt is not None
    header = open(os.path.join(os.path.dirname(build.HERE), 'include', 'kimg.h')).read()
    assert re.search(r'^int kimg_statwt\(', header, re.M)
    defines = dict(re.findall(r'^#define (KIMG_STATWT_\w+) (\d+)$', header, re.M))
    assert int(defines['KIMG_STATWT_MAX_BIN']) == statwt.MAX_BIN == 64
    assert int(defines['KIMG_STATWT_WORKSPACE_PER_ELEMENT']) == statwt.WORKSPACE_PER_ELEMENT
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
                                          statwt=None) is rec
    # host arrays straight to the collector (whose queue, None, nothing has asked for)
    assert [call[0] for call in rec.calls] == ['add', 'add', 'add', 'close'] and dataset.blocks_read == 3
    assert isinstance(rec.calls[0][2], np.ndarray) and not hasattr(rec, 'statwt_counts')


def test_loader_refuses_a_mask_of_another_length_before_any_block_is_read():
    from katsdpimager_amd import spectral
    ident = np.identity(1, np.complex64)
    for kwargs in (dict(statwt=StatWtParameters(2, fit_mask=[1] * 5)),
                   dict(statwt=StatWtParameters(2, line_ranges=[(5, 7)])),
                   # the mask spans the spectral filter's outputs, three here
                   dict(statwt=StatWtParameters(2, fit_mask=[1] * 6),
                        spectral=spectral.SpectralParameters.average(2))):
        rec, dataset = _Recorder(3 if 'spectral' in kwargs else 6), _dataset()
        with pytest.raises(ValueError):
            loader.preprocess_visibilities(dataset, rec, 0, 6, (ident, None), **kwargs)
        assert not rec.calls and dataset.blocks_read == 0
