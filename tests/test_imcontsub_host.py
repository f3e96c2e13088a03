"""Image-plane continuum subtraction without a device: the numpy twin (imcontsub.imcontsub_host)
against an independent float64 least-squares solution and against the contract's exact semantics,
the parameters object's refusals, and the argument checks of kimg_imcontsub (they run before any HIP
call).  The bound of every comparison of values is imcontsub_cases': 1e-9 S for float64 arithmetic in
another order at cond(A) <= 1e3, S the element's largest finite |I|."""
import ctypes
import os
import re

import numpy as np
import pytest

import imcontsub_cases as cases
from katsdpimager_amd import imcontsub
from katsdpimager_amd.imcontsub import ImContSubParameters


def _lstsq(cube, filled, params, frequencies=None, noise=None):
    """Per element, numpy.linalg.lstsq on the weighted design matrix of its usable fit samples:
    (model [C][M] float64, coefficients [K][M], fitted [M]) -- no code of the twin's but the tables."""
    C = cube.shape[0]
    flat = cube.reshape(C, -1).astype(np.float64)
    filled, fit, w, B, bref, min_samples = params.tables(C, filled, frequencies, noise)
    K = params.order + 1
    M = flat.shape[1]
    model = np.full((C, M), np.nan)
    a = np.full((K, M), np.nan)
    fitted = np.zeros(M, bool)
    for m in range(M):
        rows = np.flatnonzero((fit != 0) & np.isfinite(flat[:, m]))
        if len(rows) < max(K, min_samples):
            continue
        root = np.sqrt(w[rows])
        solution = np.linalg.lstsq(B[:, rows].T * root[:, None], flat[rows, m] * root, rcond=None)[0]
        a[:, m] = solution
        model[:, m] = solution @ B
        fitted[m] = True
    return model, a, fitted


def _against_lstsq(cube, filled, params, frequencies=None, noise=None):
    C = cube.shape[0]
    assert cases.worst_cond(cube, filled, params, frequencies, noise) <= 1e3
    line, maps = imcontsub.imcontsub_host_double(cube, filled, params, frequencies, noise)
    model, a, fitted = _lstsq(cube, filled, params, frequencies, noise)
    flat = cube.reshape(C, -1).astype(np.float64)
    S = cases.scale(cube, filled).reshape(-1)
    assert np.array_equal(maps['fitted'].reshape(-1), fitted)
    assert fitted.any()
    on = np.flatnonzero(filled)
    finite = np.isfinite(flat[on])
    both = finite & fitted[None, :]
    got = line.reshape(C, -1)[on]
    with np.errstate(all='ignore'):
        err = np.abs(got - (flat[on] - model[on]))
    assert (err[both] <= 1e-9 * np.broadcast_to(S, err.shape)[both]).all(), float(err[both].max())
    K = params.order + 1
    err = np.abs(maps['coefficients'].reshape(K, -1) - a)[:, fitted]
    assert (err <= 1e-9 * S[fitted]).all()
    bref = np.array([1.0, 0.0, -0.5, 0.0])[:K]
    err = np.abs(maps['continuum'].reshape(-1) - bref @ a)[fitted]
    assert (err <= 1e-9 * S[fitted]).all()
    # the rms of the residuals of the usable fit samples, n - K degrees of freedom
    fit = params.tables(C, filled, frequencies, noise)[1] != 0
    r = np.where(fit[:, None] & np.isfinite(flat), flat - model, 0.0)
    n = (fit[:, None] & np.isfinite(flat)).sum(axis=0)
    some = fitted & (n > K)
    with np.errstate(all='ignore'):
        want = np.sqrt((r * r).sum(axis=0) / (n - K))
    err = np.abs(maps['rms'].reshape(-1) - want)
    assert (err[some] <= 1e-9 * S[some]).all()
    assert some.any() or fit.sum() <= K


@pytest.mark.parametrize('C', [c for c in cases.CHANNELS if c >= 3])
def test_twin_against_least_squares(C):
    for order in cases.orders(C):
        for i, plane in enumerate(((1, 3, 5), (2, 7, 9), (1, 5, 65))):
            cube, filled, fit, frequencies, noise = cases.make_cube(C, plane, order, 100 * C + 10 * order + i)
            _against_lstsq(cube, filled, ImContSubParameters(order, fit_mask=fit))
            _against_lstsq(cube, filled, ImContSubParameters(order, fit_mask=fit, axis='frequency'),
                           frequencies)


def test_weighting():
    """Equal noises are no weighting at all, within the bound; unequal ones are the weighted
    least-squares solution."""
    C, plane, order = 33, (2, 7, 9), 2
    cube, filled, fit, frequencies, noise = cases.make_cube(C, plane, order, 7)
    none = ImContSubParameters(order, fit_mask=fit)
    weighted = ImContSubParameters(order, fit_mask=fit, weighting='noise')
    equal = np.full(C, 0.7, np.float32)
    a_line, a = imcontsub.imcontsub_host_double(cube, filled, none)
    b_line, b = imcontsub.imcontsub_host_double(cube, filled, weighted, noise=equal)
    S = cases.scale(cube, filled)
    on = filled != 0
    assert np.array_equal(np.isnan(a_line), np.isnan(b_line))
    ok = ~np.isnan(a_line[on]) & np.isfinite(a_line[on])
    with np.errstate(invalid='ignore'):
        difference = np.abs(a_line[on] - b_line[on])
    assert (difference[ok] <= 1e-9 * np.broadcast_to(S, difference.shape)[ok]).all()
    fitted = a['fitted']
    assert np.array_equal(fitted, b['fitted']) and np.array_equal(a['count'], b['count'])
    assert (np.abs(a['continuum'] - b['continuum'])[fitted] <= 1e-9 * S[fitted]).all()
    _against_lstsq(cube, filled, weighted, noise=noise)
    c_line, c = imcontsub.imcontsub_host_double(cube, filled, weighted, noise=noise)
    assert np.abs(c['continuum'] - a['continuum'])[fitted].max() > 1e-4      # (it is another fit)
    # a channel whose noise says "no weight" (0 -> inf, inf -> 0) leaves the fit
    odd = noise.copy()
    enter = np.flatnonzero(fit & filled)
    odd[enter[0]] = 0.0
    odd[enter[1]] = np.inf
    tables = weighted.tables(C, filled, noise=odd)
    assert tables[1].sum() == len(enter) - 2 and not tables[1][enter[:2]].any()
    assert np.array_equal(imcontsub.imcontsub_host_double(cube, filled, weighted, noise=odd)[1]['count'].max(),
                          len(enter) - 2)


@pytest.mark.parametrize('C', cases.CHANNELS)
def test_exact_semantics(C):
    for order in cases.orders(C):
        K = order + 1
        plane = (2, 7, 9)
        cube, filled, fit, frequencies, noise = cases.make_cube(C, plane, order, 300 * C + order)
        params = ImContSubParameters(order, fit_mask=fit)
        assert cases.worst_cond(cube, filled, params) <= 1e3
        line, maps = imcontsub.imcontsub_host(cube, filled, params)
        flat = cube.reshape(C, -1)
        enter = (fit & filled) != 0
        n = (enter[:, None] & np.isfinite(flat)).sum(axis=0)
        count = maps['count'].reshape(-1)
        assert maps['count'].dtype == np.int32 and np.array_equal(count, n)
        fitted = n >= K
        got = line.reshape(C, -1)
        on = filled != 0
        # the hand-made elements are what they were made to be
        if K >= 2:
            assert n[0] == K - 1 and not fitted[0]
        assert n[1] == K and fitted[1] and n[4] == 0 and not fitted[4]
        if enter.sum() >= K + 2:
            assert n[2] == enter.sum() - 2 and fitted[2]
        # not fitted: NaN in every filled channel, NaN maps
        assert np.isnan(got[on][:, ~fitted]).all()
        for key in ('continuum', 'rms'):
            assert np.isnan(maps[key].reshape(-1)[~fitted]).all()
            assert maps[key].dtype == np.float32 and maps[key].shape == plane
        assert maps['coefficients'].shape == (K,) + plane
        assert np.isnan(maps['coefficients'].reshape(K, -1)[:, ~fitted]).all()
        assert np.isfinite(maps['coefficients'].reshape(K, -1)[:, fitted]).all()
        assert np.isfinite(maps['continuum'].reshape(-1)[fitted]).all()
        # fitted: finite samples become finite residuals, the others keep their bits
        finite = np.isfinite(flat)
        assert np.isfinite(got[on][:, fitted][finite[on][:, fitted]]).all()
        kept = on[:, None] & fitted[None, :] & ~finite
        assert kept.any() or C < 8
        assert np.array_equal(cases.bits(got)[kept], cases.bits(flat)[kept])
        # unfilled channels are untouched
        assert np.array_equal(cases.bits(got)[~on], cases.bits(flat)[~on])
        # rms is NaN iff n <= K (or not fitted)
        assert np.array_equal(np.isnan(maps['rms'].reshape(-1)), n <= K)
        # min_samples raises the bar, never lowers it
        for least in {1, K, min(K + 2, C), C}:
            more = ImContSubParameters(order, fit_mask=fit, min_samples=least)
            _, m2 = imcontsub.imcontsub_host_double(cube, filled, more)
            assert np.array_equal(m2['fitted'].reshape(-1), n >= max(K, least))
            assert np.array_equal(m2['count'], maps['count'])
        # the rounded twin is the one rounding of the unrounded one
        d_line, d = imcontsub.imcontsub_host_double(cube, filled, params)
        with np.errstate(all='ignore'):
            assert np.array_equal(cases.bits(d['continuum'].astype(np.float32)), cases.bits(maps['continuum']))
            rounded = d_line.astype(np.float32).reshape(C, -1)
        both = on[:, None] & finite & fitted[None, :]
        assert np.array_equal(cases.bits(rounded)[both], cases.bits(got)[both])
        # the input is never written
        again = cases.make_cube(C, plane, order, 300 * C + order)[0]
        assert np.array_equal(cases.bits(cube), cases.bits(again))


def test_nan_payloads_and_quiet_nan():
    C, order = 8, 1
    fit, filled = cases.selection(C, order)
    cube = np.ones((C, 3), np.float32)
    odd = np.array([0x7fc12345, 0xffc00001, 0x7f800000], np.uint32).view(np.float32)
    line_channel = int(np.flatnonzero((fit == 0) & (filled != 0))[0])
    cube[line_channel, 0] = odd[0]
    cube[0, 1] = odd[1]
    cube[1, 1] = odd[2]
    cube[:, 2] = odd[0]
    line, maps = imcontsub.imcontsub_host(cube, filled, ImContSubParameters(order, fit_mask=fit))
    assert cases.bits(line)[line_channel, 0] == 0x7fc12345
    assert cases.bits(line)[0, 1] == 0xffc00001 and cases.bits(line)[1, 1] == 0x7f800000
    on = filled != 0
    assert (cases.bits(line)[on, 2] == 0x7fc00000).all()        # not fitted: the quiet NaN
    assert (cases.bits(line)[~on, 2] == 0x7fc12345).all()       # not filled: untouched
    assert maps['count'].tolist() == [int((fit & filled).sum()), int((fit & filled).sum()) - 2, 0]


@pytest.mark.parametrize('order', [0, 1, 2, 3])
def test_exact_fits(order):
    """A pure polynomial of the fitted order leaves nothing, and its continuum map is the polynomial
    at mid-band -- by channel index and by uneven frequencies."""
    C, M = 33, 40
    rng = np.random.default_rng(order)
    fit, filled = cases.selection(C, order)
    frequencies = 1.4e9 + 1.0e6 * (np.arange(C) + 0.3 * np.sin(np.arange(C)))
    for axis, position in (('channel', np.arange(C, dtype=np.float64)), ('frequency', frequencies)):
        x = (position - position.min() - (position.max() - position)) / (position.max() - position.min())
        coefficients = rng.normal(0.0, 2.0, (order + 1, M))
        cube = sum(coefficients[k][None, :] * x[:, None] ** k for k in range(order + 1)).astype(np.float64)
        data = cube.astype(np.float32)
        # (the float32 input is the polynomial only to 2^-24: fit what was rounded)
        params = ImContSubParameters(order, fit_mask=fit, axis=axis)
        exact = np.polynomial.polynomial.polyfit(x[(fit & filled) != 0], data[(fit & filled) != 0].astype(np.float64), order)
        line, maps = imcontsub.imcontsub_host_double(data, filled, params, frequencies)
        S = cases.scale(data, filled)
        on = filled != 0
        want = data[on].astype(np.float64) - np.polynomial.polynomial.polyval(x[on], exact).T
        assert (np.abs(line[on] - want) <= 1e-9 * S[None, :]).all()
        assert (np.abs(line[on]) <= 2.0 ** -23 * S[None, :]).all()
        assert (np.abs(maps['continuum'] - exact[0]) <= 1e-9 * S).all()      # the polynomial at x = 0
        assert (np.abs(maps['continuum'] - coefficients[0]) <= 2.0 ** -22 * S).all()


def test_exact_fit_of_exact_data():
    """Samples on a 1/64 grid of a polynomial with dyadic coefficients are exact in float32: the line
    cube is within 1e-9 S of zero and the continuum map is the polynomial at mid-band."""
    C, M = 33, 12
    x = (2.0 * np.arange(C) - (C - 1)) / (C - 1)           # k / 16: exact
    rng = np.random.default_rng(3)
    for order in range(4):
        fit, filled = cases.selection(C, order)
        coefficients = rng.integers(-8, 9, (order + 1, M)).astype(np.float64) / 4.0
        cube = sum(coefficients[k][None, :] * x[:, None] ** k for k in range(order + 1))
        data = cube.astype(np.float32)
        assert np.array_equal(data.astype(np.float64), cube)
        line, maps = imcontsub.imcontsub_host_double(data, filled, ImContSubParameters(order, fit_mask=fit))
        S = cases.scale(data, filled)
        S = np.maximum(S, 1.0)
        on = filled != 0
        assert (np.abs(line[on]) <= 1e-9 * S[None, :]).all()
        assert (np.abs(maps['continuum'] - coefficients[0]) <= 1e-9 * S).all()
        assert (maps['rms'] <= 1e-9 * S).all()


def test_parameter_refusals():
    mask = [1, 1, 0, 0, 1, 1, 1, 1]
    for bad in (-1, 4, 1.5, 'a', None):
        with pytest.raises(ValueError):
            ImContSubParameters(bad, fit_mask=mask)
    with pytest.raises(ValueError):
        ImContSubParameters(1)                                          # neither spelling
    with pytest.raises(ValueError):
        ImContSubParameters(1, fit_mask=mask, line_ranges=[(2, 4)])     # both
    with pytest.raises(ValueError):
        ImContSubParameters(3, fit_mask=[1, 1, 1, 0, 0])                # too few channels left
    with pytest.raises(ValueError):
        ImContSubParameters(1, line_ranges=[(0, 7)]).mask(8)
    with pytest.raises(ValueError):
        ImContSubParameters(1, line_ranges=[(2, 9)]).mask(8)            # beyond the band
    with pytest.raises(ValueError):
        ImContSubParameters(1, fit_mask=mask, axis='velocity')
    with pytest.raises(ValueError):
        ImContSubParameters(1, fit_mask=mask, weighting='robust')
    for bad in (0, 9, 2.5, 'a'):
        with pytest.raises(ValueError):
            ImContSubParameters(1, fit_mask=mask, min_samples=bad)
    with pytest.raises(ValueError):
        ImContSubParameters(1, line_ranges=[(2, 4)], min_samples=9).mask(8)
    ImContSubParameters(1, line_ranges=[(2, 4)], min_samples=8).mask(8)
    cube = np.zeros((8, 5), np.float32)
    filled = np.ones(8, np.uint8)
    noise = np.ones(8, np.float32)
    # too few channels left once filled and the weights are folded in
    few = filled.copy()
    few[[0, 1, 4, 5, 6]] = 0
    with pytest.raises(ValueError):
        imcontsub.imcontsub_host(cube, few, ImContSubParameters(1, fit_mask=mask))
    # noise missing for a filled fit channel; not for a line channel or one that is not filled
    weighted = ImContSubParameters(1, fit_mask=mask, weighting='noise')
    with pytest.raises(ValueError):
        imcontsub.imcontsub_host(cube, filled, weighted)
    missing = noise.copy()
    missing[5] = np.nan
    with pytest.raises(ValueError):
        imcontsub.imcontsub_host(cube, filled, weighted, noise=missing)
    with pytest.raises(ValueError):
        imcontsub.imcontsub_host(cube, filled, weighted, noise=noise[:7])
    missing = noise.copy()
    missing[[2, 5]] = np.nan
    holes = filled.copy()
    holes[5] = 0
    imcontsub.imcontsub_host(cube, holes, weighted, noise=missing)
    # frequencies: needed on that axis, one per channel, finite
    by_frequency = ImContSubParameters(1, fit_mask=mask, axis='frequency')
    with pytest.raises(ValueError):
        imcontsub.imcontsub_host(cube, filled, by_frequency)
    with pytest.raises(ValueError):
        imcontsub.imcontsub_host(cube, filled, by_frequency, frequencies=np.arange(7.0))
    with pytest.raises(ValueError):
        imcontsub.imcontsub_host(cube, filled, ImContSubParameters(1, fit_mask=mask), frequencies=np.arange(9.0))
    with pytest.raises(ValueError):
        imcontsub.imcontsub_host(cube, filled, by_frequency, frequencies=[1.0] * 7 + [np.nan])
    # the cube and its tables
    with pytest.raises(TypeError):
        imcontsub.imcontsub_host(cube.astype(np.float64), filled, by_frequency, np.arange(8.0))
    with pytest.raises(ValueError):
        imcontsub.imcontsub_host(cube[:, 0], filled, ImContSubParameters(1, fit_mask=mask))
    with pytest.raises(ValueError):
        imcontsub.imcontsub_host(cube, filled[:7], ImContSubParameters(1, fit_mask=mask))
    with pytest.raises(ValueError):
        imcontsub.imcontsub_host(cube[:7], filled[:7], ImContSubParameters(1, fit_mask=mask))
    with pytest.raises(TypeError):
        imcontsub.ImContSubTemplate(None, object())


def test_repr():
    assert repr(ImContSubParameters(2, line_ranges=[(3, 9)])) == 'ImContSubParameters(2, line_ranges=[(3, 9)])'
    text = repr(ImContSubParameters(0, fit_mask=[1, 0, 1], axis='frequency', weighting='noise', min_samples=2))
    assert text == ("ImContSubParameters(0, fit_mask=[1, 0, 1], axis='frequency', weighting='noise', "
                    "min_samples=2)")


def test_argument_errors_return_their_codes():
    from katsdpimager_amd import _lib
    C, M = 8, 64
    memory = np.full(2 * C * M + 8 * M, 7.0, np.float32)
    tables = np.ones(5 * C, np.float64)
    base = memory.ctypes.data
    base += -base % 16
    assert tables.ctypes.data % 8 == 0
    checked = cases.abi_errors(_lib.lib(), base, base + 4 * C * M, tables.ctypes.data,
                               base + 8 * C * M, C, M)
    assert checked == 37
    assert (memory == 7.0).all() and (tables == 1.0).all()


def test_symbol_is_declared_exported_and_prototyped():
    from katsdpimager_amd import _lib, build, cube
    assert 'imcontsub.hip' in build.SOURCES
    for name in ('imcontsub.hip', 'kimg_cube_column.h', 'kimg_cholesky.h'):
        assert os.path.exists(os.path.join(build.CSRC, name))
    assert 'kimg_imcontsub' in _lib.PROTOTYPES
    restype, argtypes = _lib.PROTOTYPES['kimg_imcontsub']
    assert restype is ctypes.c_int and len(argtypes) == 24
    assert _lib.lib().kimg_imcontsub is not None
    header = open(os.path.join(os.path.dirname(build.HERE), 'include', 'kimg.h')).read()
    declaration = re.search(r'^int kimg_imcontsub\(([^;]*)\);', header, re.M).group(1)
    assert declaration.count(',') + 1 == 24
    defines = dict(re.findall(r'^#define (KIMG_IMCONTSUB_\w+) (\d+)$', header, re.M))
    assert int(defines.pop('KIMG_IMCONTSUB_MAX_ORDER')) == imcontsub.MAX_ORDER == 3
    assert {'KIMG_IMCONTSUB_' + key.upper(): str(bit) for key, bit in imcontsub.OUTPUT_BITS.items()} == defines
    assert imcontsub.MAX_CHANNELS == cube.MAX_CHANNELS == 4096
    # the two shared headers are shared: each is included by the two units that use it
    for name, units in (('kimg_cube_column.h', ('moments.hip', 'imcontsub.hip')),
                        ('kimg_cholesky.h', ('contsub.hip', 'imcontsub.hip'))):
        for unit in units:
            assert '#include "{}"'.format(name) in open(os.path.join(build.CSRC, unit)).read()
    assert _lib.lib().kimg_version() == _lib.VERSION == 5
