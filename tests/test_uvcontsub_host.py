"""UV-plane continuum subtraction without a device: the parameters object, the Legendre basis, the
argument checks of kimg_uvcontsub (they run before any HIP call), and the numpy twin
(continuum.uvcontsub_host, the executable form of the contract in include/kimg.h) against an
independent least-squares solve, on exact polynomials and on samples that cannot be fitted."""
import ctypes

import numpy as np
import pytest

import band_cases as bands
from katsdpimager_amd import continuum
from katsdpimager_amd.continuum import UVContSubParameters, legendre_basis, uvcontsub_host

EINVAL, EUNSUPPORTED = -10001, -10002


# ---- basis ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [1, 2, 5, 16, 24])
def test_basis_is_legendre_of_the_channel_index(C):
    x = (2.0 * np.arange(C) - (C - 1)) / (C - 1) if C > 1 else np.zeros(1)
    for order in range(4):
        basis = legendre_basis(order, C)
        assert basis.shape == (order + 1, C) and basis.dtype == np.float64
        for k in range(order + 1):
            want = np.polynomial.legendre.legval(x, np.eye(4)[k])
            np.testing.assert_allclose(basis[k], want, rtol=0, atol=4e-16)
    if C > 1:
        assert basis[1, 0] == -1.0 and basis[1, -1] == 1.0


def test_basis_of_frequencies_puts_the_end_channels_on_plus_and_minus_one():
    freq = 1.4e9 + 26123.7 * np.arange(11) ** 1.3         # (unevenly spaced)
    basis = legendre_basis(3, 11, freq)
    assert basis[1, 0] == -1.0 and basis[1, -1] == 1.0
    offset = freq - freq[0]         # (2 f - (f0 + f1) would lose the band's width in 2 f's rounding)
    x = 2 * offset / offset[-1] - 1
    for k in range(4):
        np.testing.assert_allclose(basis[k], np.polynomial.legendre.legval(x, np.eye(4)[k]),
                                   rtol=0, atol=1e-14)
    down = legendre_basis(1, 11, freq[::-1])                # a band that runs downwards
    assert down[1, 0] == 1.0 and down[1, -1] == -1.0
    np.testing.assert_array_equal(legendre_basis(2, 3, [5.0, 5.0, 5.0])[1], 0.0)
    with pytest.raises(ValueError):
        legendre_basis(1, 4, freq)
    with pytest.raises(ValueError):
        legendre_basis(4, 8)


# ---- refusals ---------------------------------------------------------------------------------------
def test_parameters_refuse():
    ok = UVContSubParameters(3, fit_mask=[1, 1, 0, 1, 1])
    assert ok.order == 3 and ok.mask(5).tolist() == [1, 1, 0, 1, 1]
    ranges = UVContSubParameters(1, line_ranges=[(6, 10)])
    assert ranges.mask(16).tolist() == [1] * 6 + [0] * 4 + [1] * 6
    with pytest.raises(ValueError):
        UVContSubParameters(4, fit_mask=np.ones(16))                # order 4
    with pytest.raises(ValueError):
        UVContSubParameters(-1, fit_mask=np.ones(16))
    with pytest.raises(ValueError):
        UVContSubParameters(1.5, fit_mask=np.ones(16))
    with pytest.raises(ValueError):
        UVContSubParameters(0, fit_mask=np.zeros(8))                # an empty mask
    with pytest.raises(ValueError):
        UVContSubParameters(0, fit_mask=[])
    with pytest.raises(ValueError):
        UVContSubParameters(2, fit_mask=[1, 0, 0, 1, 0])            # fewer line-free channels than K
    with pytest.raises(ValueError):
        UVContSubParameters(1, fit_mask=np.ones(8), line_ranges=[(2, 4)])   # both
    with pytest.raises(ValueError):
        UVContSubParameters(1)                                      # neither
    with pytest.raises(ValueError):
        UVContSubParameters(1, fit_mask=np.ones(8), frequencies=np.arange(7.0))
    with pytest.raises(ValueError):
        ranges.mask(8)                          # the range lies beyond the channels
    with pytest.raises(ValueError):
        UVContSubParameters(2, line_ranges=[(1, 7)]).mask(8)        # 2 channels remain, 3 needed
    with pytest.raises(ValueError):
        ok.mask(6)


def test_entry_point_refuses_before_any_hip_call():
    from katsdpimager_amd import _lib
    fn = _lib.lib().kimg_uvcontsub
    one = ctypes.c_void_p(1)

    def call(C, order, mask, vis=one, weights=one, basis=one, counts=one, plane=8, vp=8, wp=8):
        m = np.asarray(mask, np.uint8)
        return fn(vis, vp, weights, wp, C, plane, m.ctypes.data_as(ctypes.c_void_p) if m.size else None,
                  basis, order, counts, None)
    full = np.ones(16, np.uint8)
    assert call(16, 4, full) == EINVAL                  # order 4
    assert call(16, -1, full) == EINVAL
    assert call(0, 0, full) == EINVAL                   # no channels
    assert call(16, 0, np.zeros(16)) == EUNSUPPORTED    # an empty mask
    assert call(5, 2, [1, 0, 0, 1, 0]) == EUNSUPPORTED  # fewer line-free channels than K
    assert call(5, 2, [1, 0, 0, 1, 0], vis=None, weights=None, basis=None, counts=None) == EUNSUPPORTED
    assert call(16, 1, []) == EINVAL                    # no mask at all
    assert call(continuum.MAX_CHANNELS + 1, 1, np.ones(continuum.MAX_CHANNELS + 1)) == EUNSUPPORTED
    for null in ('vis', 'weights', 'basis', 'counts'):
        assert call(16, 1, full, **{null: None}) == EINVAL
    assert call(16, 1, full, plane=-1) == EINVAL
    assert call(16, 1, full, vp=7) == EINVAL            # channels would overlap
    assert call(16, 1, full, wp=7) == EINVAL
    assert call(16, 1, full, plane=0, vp=0, wp=0) == 0  # nothing to do, nothing launched


# ---- the twin ---------------------------------------------------------------------------------------
def _random_block(rng, C, N, Q, zero_fraction=0.2):
    vis = ((rng.normal(size=(C, N, Q)) + 1j * rng.normal(size=(C, N, Q))) * 3.0).astype(np.complex64)
    weights = rng.uniform(0.5, 2.0, (C, N, Q)).astype(np.float32)
    weights[rng.random((C, N, Q)) < zero_fraction] = 0.0
    return vis, weights


@pytest.mark.parametrize('C,order,mask', [
    (24, 3, [1] * 9 + [0] * 6 + [1] * 9), (5, 3, [1] * 5), (16, 1, [1] * 6 + [0] * 4 + [1] * 6),
    (7, 2, [1, 1, 0, 0, 0, 1, 1]), (1, 0, [1]), (12, 0, [0, 1] * 6),
    # past one word of the device's bit mask (band_cases.py)
    (65, 3, bands.straddle(65)), (65, 2, bands.word0_empty(65))])
def test_twin_against_an_independent_solve(C, order, mask):
    """For every sample the model of the twin (input - output, in float64) against numpy's lstsq
    on the sqrt(w)-scaled system, to 1e-10 of the sample's largest |v|."""
    rng = np.random.default_rng(100 * C + order)
    N, Q = 37, 2
    vis, weights = _random_block(rng, C, N, Q)
    vis[min(3, C - 1), 5, 0] = np.nan               # a NaN in a fit channel is left out of the fit
    weights[0, 6, 1] = -1.0                     # and so is a negative weight
    params = UVContSubParameters(order, fit_mask=mask)
    out, new_weights, fitted = continuum.uvcontsub_host_double(vis, weights, params)
    B = legendre_basis(order, C)
    K = order + 1
    fit = np.asarray(mask, bool)
    checked = 0
    for n in range(N):
        for q in range(Q):
            v = vis[:, n, q].astype(np.complex128)
            usable = fit & (weights[:, n, q] > 0) & np.isfinite(v)
            if usable.sum() < K:
                assert not fitted[n, q]
                continue
            assert fitted[n, q]
            root = np.sqrt(weights[usable, n, q].astype(np.float64))
            coeff = np.linalg.lstsq(B[:, usable].T * root[:, None], v[usable] * root, rcond=None)[0]
            model = coeff @ B
            finite = np.isfinite(v)
            S = np.abs(v[finite]).max()
            got = v[finite] - out[finite, n, q]
            assert np.abs(got - model[finite]).max() <= 1e-10 * S
            checked += 1
    assert checked > N
    rounded, w2, counts = uvcontsub_host(vis, weights, params)
    assert rounded.dtype == np.complex64 and w2.dtype == np.float32
    assert counts == (int(fitted.sum()), int((~fitted).sum()))
    np.testing.assert_array_equal(w2, new_weights)
    np.testing.assert_array_equal(w2[:, fitted], weights[:, fitted])


@pytest.mark.parametrize('order', [0, 1, 2, 3])
@pytest.mark.parametrize('use_frequencies', [False, True])
def test_exact_polynomial_leaves_rounding_and_the_line(order, use_frequencies):
    """A continuum that is a polynomial of degree <= order in x plus a line confined to the
    masked-out channels: the fit channels come out as rounding (<= 2^-23 S), the line channels as
    the line within 2^-23 S."""
    rng = np.random.default_rng(7 + order)
    C, N, Q = 20, 50, 2
    freq = 1.0e9 + 1.0e6 * np.cumsum(rng.uniform(0.5, 1.5, C)) if use_frequencies else None
    x = legendre_basis(1, C, freq)[1]
    coeff = rng.normal(size=(order + 1, N, Q)) + 1j * rng.normal(size=(order + 1, N, Q))
    cont = sum(coeff[k][None] * x[:, None, None] ** k for k in range(order + 1))
    line = np.zeros((C, N, Q), np.complex128)
    line[8:12] = 0.3 * (rng.normal(size=(4, N, Q)) + 1j * rng.normal(size=(4, N, Q)))
    vis = (cont + line).astype(np.complex64)
    weights = rng.uniform(0.5, 2.0, (C, N, Q)).astype(np.float32)
    params = UVContSubParameters(order, line_ranges=[(8, 12)], frequencies=freq)
    out, w2, counts = uvcontsub_host(vis, weights, params)
    assert counts == (N * Q, 0)
    np.testing.assert_array_equal(w2, weights)
    S = np.abs(vis).max(axis=0)
    free = params.mask(C).astype(bool)
    assert (np.abs(out[free]) <= 2.0 ** -23 * S).all()
    assert (np.abs(out[~free] - line[~free]) <= 2.0 ** -23 * S).all()


def test_samples_that_cannot_be_fitted_are_flagged():
    """m < K: vis kept bit for bit, every weight 0, counted; m == K exactly is fitted (and then
    interpolates its K channels); NaN and zero-weight channels do not count towards m."""
    rng = np.random.default_rng(5)
    C, N, Q = 9, 6, 1
    order, K = 2, 3
    mask = np.array([1, 1, 1, 0, 0, 0, 1, 1, 1], np.uint8)
    vis, weights = _random_block(rng, C, N, Q, zero_fraction=0.0)
    # sample 0: all six fit channels usable
    # sample 1: exactly K usable (three knocked out in three different ways)
    weights[0, 1, 0] = 0.0
    weights[1, 1, 0] = -2.0
    vis[6, 1, 0] = complex(np.nan, 1.0)
    # sample 2: K - 1 usable
    weights[[0, 1, 2], 2, 0] = 0.0
    vis[8, 2, 0] = complex(1.0, np.inf)
    # sample 3: none usable; sample 4: NaN only in a LINE channel (does not matter to m)
    weights[:, 3, 0] = 0.0
    vis[4, 4, 0] = np.nan
    # sample 5: usable everywhere except the line channels have weight 0 (they are not counted anyway)
    weights[3:6, 5, 0] = 0.0
    params = UVContSubParameters(order, fit_mask=mask)
    out, w2, counts = uvcontsub_host(vis, weights, params)
    assert counts == (4, 2)
    for n in (2, 3):
        np.testing.assert_array_equal(out[:, n].view(np.uint32), vis[:, n].view(np.uint32))
        assert (w2[:, n] == 0).all()
    for n in (0, 1, 4, 5):
        np.testing.assert_array_equal(w2[:, n], weights[:, n])
    # m == K: the parabola goes through the three usable channels
    usable = [2, 7, 8]
    S = np.abs(vis[np.isfinite(vis[:, 1, 0]), 1, 0]).max()
    assert np.abs(out[usable, 1, 0]).max() <= 2.0 ** -23 * S
    assert np.abs(out[0, 1, 0]) > 1e-3          # (an unusable fit channel is still subtracted from)
    assert np.isnan(out[6, 1, 0].real)          # IEEE: NaN in, NaN out
    assert np.isnan(out[4, 4, 0].real) and np.isfinite(out[[0, 1, 2, 3, 5, 6, 7, 8], 4, 0]).all()


# ---- the long-band blocks of test_uvcontsub_gpu.py hold what they were made for ----------------------
def test_band_masks_reach_every_seam():
    for C in bands.CHANNELS:
        bands.self_check(C)
    C = continuum.MAX_CHANNELS
    mask = bands.limit_mask(C)
    assert np.flatnonzero(mask == 0).tolist() == [8191, 8192, C - 7, C - 1]
    assert bands.packed(mask)[[255, 256, 511]].tolist() == [0x7fffffff, 0xfffffffe, 0x7dffffff]


@pytest.mark.parametrize('C', bands.CHANNELS)
def test_long_band_cases_are_well_conditioned_and_hold_their_samples(C):
    """What test_uvcontsub_gpu.test_device_against_twin_past_one_mask_word asserts of its inputs, with
    the twin alone: cond(A) <= 1e3, a sample that is fitted and one that is not, and the hand-made
    samples' surviving channels outside word 0 of the mask wherever K fit channels lie there."""
    import test_uvcontsub_gpu as device_cases
    for order in range(4):
        K = order + 1
        cases = bands.masks(C, least=K)
        assert len(cases) >= 4 and all(mask.sum() >= K for _, mask in cases)
        for i, (name, mask) in enumerate(cases):
            N, Q = bands.PLANES[i % 2]
            vis, weights, params, pool = device_cases.seam_inputs(C, order, mask, N, Q, 7000 * C + 10 * i)
            assert device_cases._cond(weights, vis, C, order, mask, params.frequencies) <= 1e3
            x = continuum.legendre_basis(1, C, params.frequencies)[1]
            assert x[0] == -1.0 and x[-1] == 1.0 and (np.diff(x) > 0).all()
            _, new_weights, fitted = continuum.uvcontsub_host_double(vis, weights, params)
            fitted, v, w = fitted.reshape(-1), vis.reshape(C, -1), weights.reshape(C, -1)
            usable = mask.astype(bool)[:, None] & (w > 0) & np.isfinite(v.real) & np.isfinite(v.imag)
            assert not fitted[3] and usable[:, 3].sum() == K - 1
            assert fitted[5] and usable[:, 5].sum() == K
            assert usable[:, 40].sum() == usable[:, 41].sum() == mask.sum() - 1
            assert fitted[40] == fitted[41] == (mask.sum() - 1 >= K)
            if (np.flatnonzero(mask) >= bands.WORD).sum() >= K:
                assert pool.min() >= bands.WORD
                assert np.flatnonzero(usable[:, 5]).min() >= bands.WORD
                assert K == 1 or np.flatnonzero(usable[:, 3]).min() >= bands.WORD
