"""Spectral smoothing and channel averaging without a device: the parameters object, the numpy twin
(spectral.filter_host, the executable form of the contract in include/kimg.h) against truths that do
not share its code, the noise it promises, the argument checks of kimg_spectral_filter (they run
before any HIP call), the ABI surface, and the loader's keyword."""
import ctypes
import os
import re

import numpy as np
import pytest

from katsdpimager_amd import loader, spectral
from katsdpimager_amd.spectral import SpectralParameters, filter_host, filter_host_double

EINVAL, EUNSUPPORTED = -10001, -10002
HANNING = (0.25, 0.5, 0.25)


def _block(rng, C, N, Q):
    vis = ((rng.normal(size=(C, N, Q)) + 1j * rng.normal(size=(C, N, Q))) * 3.0).astype(np.complex64)
    weights = rng.uniform(0.5, 2.0, (C, N, Q)).astype(np.float32)
    return vis, weights


# ---- the parameters object --------------------------------------------------------------------------
def test_parameters_and_their_derived_values():
    p = SpectralParameters()
    assert p.taps.tolist() == [1.0] and p.bin == 1 and p.min_coverage == 0.5
    g, offset, step = p.coefficients()
    assert g.tolist() == [1.0] and (offset, step) == (0, 1)
    h = SpectralParameters.hanning()
    assert h.taps.tolist() == [0.25, 0.5, 0.25] and h.bin == 1
    g, offset, step = SpectralParameters.hanning(bin=2).coefficients()
    assert g.dtype == np.float64 and g.tolist() == [0.25, 0.75, 0.75, 0.25] and (offset, step) == (1, 2)
    g, offset, step = SpectralParameters.average(4).coefficients()
    assert g.tolist() == [1.0] * 4 and (offset, step) == (0, 4)
    assert SpectralParameters.average(4).min_sum() == 2.0
    g, offset, step = SpectralParameters(np.ones(9), 64).coefficients()
    assert len(g) == 72 and offset == 4 and step == 64
    assert SpectralParameters.average(3).output_channels(7) == 2
    assert SpectralParameters.hanning().output_channels(1) == 1
    freq = 1.4e9 + 1e5 * np.arange(7.0) ** 1.1
    out = SpectralParameters.hanning(bin=2).output_frequencies(freq)
    assert out.dtype == np.float64 and out.shape == (3,)
    np.testing.assert_allclose(out, [(freq[0] + freq[1]) / 2, (freq[2] + freq[3]) / 2,
                                     (freq[4] + freq[5]) / 2], rtol=1e-15)
    np.testing.assert_array_equal(SpectralParameters.hanning().output_frequencies(freq), freq)


@pytest.mark.parametrize('kwargs', [
    dict(taps=(0.5, 0.5)),                                  # even K
    dict(taps=np.ones(11)),                                 # K = 11
    dict(taps=(0.25, 0.5, -0.25)),                          # a negative tap
    dict(taps=(0.25, 0.5, np.nan)),
    dict(taps=(0.25, 0.5, np.inf)),
    dict(taps=(0.5, 0.0, 0.5)),                             # a zero centre tap
    dict(taps=()),
    dict(bin=0), dict(bin=65), dict(bin=1.5), dict(bin='a'),
    dict(min_coverage=0.0), dict(min_coverage=1.5), dict(min_coverage=np.nan),
    dict(min_coverage=-0.1),
])
def test_parameters_refuse(kwargs):
    with pytest.raises(ValueError):
        SpectralParameters(**kwargs)


def test_fewer_channels_than_the_bin_are_refused():
    p = SpectralParameters.average(4)
    with pytest.raises(ValueError):
        p.output_channels(3)
    with pytest.raises(ValueError):
        p.output_frequencies(np.arange(3.0))
    vis, weights = _block(np.random.default_rng(0), 3, 2, 1)
    with pytest.raises(ValueError):
        filter_host(vis, weights, p)
    with pytest.raises(TypeError):
        filter_host(vis.astype(np.complex128), weights, SpectralParameters())
    with pytest.raises(ValueError):
        filter_host(vis, weights[:2], SpectralParameters())


# ---- the twin against truths that do not share its code ---------------------------------------------
@pytest.mark.parametrize('params', [SpectralParameters.hanning(), SpectralParameters.average(4),
                                    SpectralParameters.hanning(bin=3)])
def test_constant_spectrum_stays_that_constant(params):
    rng = np.random.default_rng(3)
    C, N, Q = 13, 11, 2
    _, weights = _block(rng, C, N, Q)
    value = (rng.normal(size=(N, Q)) + 1j * rng.normal(size=(N, Q))).astype(np.complex64)
    vis = np.broadcast_to(value, (C, N, Q)).copy()
    out, w, counts = filter_host(vis, weights, params)
    C_out = C // params.bin
    assert out.shape == (C_out, N, Q) and out.dtype == np.complex64 and w.dtype == np.float32
    assert counts == (C_out * N * Q, 0)
    # (N / S1 is the constant up to the rounding of the float64 sums; one float32 rounding on top)
    assert np.abs(out - value[None]).max() <= 2.0 ** -23 * np.abs(value).max()
    assert (w > 0).all()


def test_unit_weights_under_hanning():
    C, N, Q = 6, 3, 1
    vis, _ = _block(np.random.default_rng(4), C, N, Q)
    out, w, counts = filter_host(vis, np.ones((C, N, Q), np.float32), SpectralParameters.hanning())
    assert counts == (C * N * Q, 0)
    np.testing.assert_array_equal(w[1:-1], np.float32(1 / 0.375))
    edge = np.float32(0.75 ** 2 / (0.25 ** 2 + 0.5 ** 2))
    np.testing.assert_array_equal(w[0], edge)
    np.testing.assert_array_equal(w[-1], edge)
    v = vis.astype(np.complex128)
    np.testing.assert_allclose(out[2], 0.25 * v[1] + 0.5 * v[2] + 0.25 * v[3], rtol=2.0 ** -23)
    np.testing.assert_allclose(out[0], (0.5 * v[0] + 0.25 * v[1]) / 0.75, rtol=2.0 ** -23)


@pytest.mark.parametrize('n', [1, 2, 5])
def test_average_is_the_weighted_mean_with_the_sum_of_weights(n):
    rng = np.random.default_rng(10 + n)
    C, N, Q = 5 * n + (n - 1), 9, 3
    vis, weights = _block(rng, C, N, Q)
    out, w, kept = filter_host_double(vis, weights, SpectralParameters.average(n))
    assert kept.all() and out.shape == (5, N, Q)
    v = vis[:5 * n].astype(np.complex128).reshape(5, n, N, Q)
    ww = weights[:5 * n].astype(np.float64).reshape(5, n, N, Q)
    sum_w = np.einsum('oinq->onq', ww)
    want = np.einsum('oinq,oinq->onq', ww, v) / sum_w
    np.testing.assert_allclose(out, want, rtol=1e-14)
    np.testing.assert_allclose(w, sum_w, rtol=1e-14)


def test_hanning_with_a_bin_is_hanning_then_averaging():
    """Two separate dense matrix products in float64: H [C][C] (Hanning, cut at the band edges), then
    A [C_out][C] (the box).  With every input usable, N = A H (w v), S1 = A H w and
    S2 = (A H)^2 w, the square taken entry by entry."""
    rng = np.random.default_rng(6)
    C, N, Q = 9, 7, 2
    vis, weights = _block(rng, C, N, Q)
    H = np.zeros((C, C))
    for c in range(C):
        for d, t in zip((-1, 0, 1), HANNING):
            if 0 <= c + d < C:
                H[c, c + d] = t
    A = np.zeros((C // 2, C))
    for o in range(C // 2):
        A[o, 2 * o:2 * o + 2] = 1.0
    w = weights.astype(np.float64).reshape(C, -1)
    v = vis.astype(np.complex128).reshape(C, -1)
    smoothed_wv = H @ (w * v)
    smoothed_w = H @ w
    numer = A @ smoothed_wv
    S1 = A @ smoothed_w
    S2 = (A @ H) ** 2 @ w
    out, new_w, kept = filter_host_double(vis, weights, SpectralParameters.hanning(bin=2))
    assert kept.all()
    np.testing.assert_allclose(out.reshape(C // 2, -1), numer / S1, rtol=1e-13)
    np.testing.assert_allclose(new_w.reshape(C // 2, -1), S1 * S1 / S2, rtol=1e-13)


def test_trailing_channels_enter_only_through_the_smoothing():
    rng = np.random.default_rng(8)
    vis, weights = _block(rng, 7, 4, 1)
    changed = vis.copy()
    changed[6] += 1.0
    for params, enters in ((SpectralParameters.hanning(bin=2), True), (SpectralParameters.average(2), False)):
        a, wa, _ = filter_host(vis, weights, params)
        b, wb, _ = filter_host(changed, weights, params)
        assert a.shape == (3, 4, 1)
        np.testing.assert_array_equal(a[:2], b[:2])
        assert (a[2] != b[2]).all() == enters and (a[2] != b[2]).any() == enters
        np.testing.assert_array_equal(wa, wb)


@pytest.mark.parametrize('bad', ['zero', 'negative', 'nan', 'inf'])
def test_an_unusable_input_is_left_out_and_the_rest_renormalised(bad):
    rng = np.random.default_rng(9)
    C = 5
    vis, weights = _block(rng, C, 1, 1)
    if bad == 'zero':
        weights[2] = 0.0
    elif bad == 'negative':
        weights[2] = -1.0
    elif bad == 'nan':
        vis[2] = complex(np.nan, 1.0)
    else:
        vis[2] = complex(1.0, -np.inf)
    out, w, kept = filter_host_double(vis, weights, SpectralParameters.hanning())
    v = vis[:, 0, 0].astype(np.complex128)
    ww = weights[:, 0, 0].astype(np.float64)
    assert kept[[0, 1, 3, 4]].all()
    # output 1: inputs 0 (1/4) and 1 (1/2); output 3: inputs 3 (1/2) and 4 (1/4)
    for o, (i, j) in ((1, (0, 1)), (3, (3, 4))):
        gi, gj = (0.25, 0.5) if o == 1 else (0.5, 0.25)
        s1 = gi * ww[i] + gj * ww[j]
        np.testing.assert_allclose(out[o, 0, 0], (gi * ww[i] * v[i] + gj * ww[j] * v[j]) / s1, rtol=1e-14)
        np.testing.assert_allclose(w[o, 0, 0], s1 * s1 / (gi * gi * ww[i] + gj * gj * ww[j]), rtol=1e-14)
    # output 2 has lost its centre: coverage 0.5, exactly at the default threshold, is kept ...
    assert kept[2, 0, 0]
    s1 = 0.25 * ww[1] + 0.25 * ww[3]
    np.testing.assert_allclose(out[2, 0, 0], 0.25 * (ww[1] * v[1] + ww[3] * v[3]) / s1, rtol=1e-14)
    # ... and one step above it is flagged
    above = SpectralParameters.hanning(min_coverage=np.nextafter(0.5, 1.0))
    out2, w2, counts = filter_host(vis, weights, above)
    assert counts == (4, 1)
    assert out2[2, 0, 0] == 0 and w2[2, 0, 0] == 0
    np.testing.assert_array_equal(out2[[0, 1, 3, 4]], out.astype(np.complex64)[[0, 1, 3, 4]])


def test_a_window_without_usable_inputs_is_flagged_with_zeros():
    rng = np.random.default_rng(12)
    vis, weights = _block(rng, 8, 3, 2)
    weights[2:4, 1, 0] = 0.0
    vis[2, 1, 1] = np.nan
    weights[3, 1, 1] = -2.0
    out, w, counts = filter_host(vis, weights, SpectralParameters.average(2))
    assert counts == (4 * 3 * 2 - 2, 2)
    for q in (0, 1):
        assert out[1, 1, q] == 0 and w[1, 1, q] == 0
        assert not np.signbit(w[1, 1, q]) and not np.signbit(out[1, 1, q].real)
    assert np.isfinite(out.real).all() and np.isfinite(out.imag).all()
    assert (w[[0, 2, 3]] > 0).all()


def test_noise_of_the_output_is_what_its_weight_says():
    """20 000 samples of unit-variance noise scaled by 1 / sqrt(w), random w, through Hanning + bin 2:
    sqrt(w_out) Re(v_out) has variance 1 within 5 % (five standard errors of sqrt(2 / 20000) = 1 %)."""
    rng = np.random.default_rng(2024)
    C, N = 9, 5000
    weights = rng.uniform(0.3, 3.0, (C, N, 1)).astype(np.float32)
    sigma = 1.0 / np.sqrt(weights.astype(np.float64))
    vis = ((rng.normal(size=(C, N, 1)) + 1j * rng.normal(size=(C, N, 1))) * sigma).astype(np.complex64)
    out, w, counts = filter_host(vis, weights, SpectralParameters.hanning(bin=2))
    assert out.size == 20000 and counts == (20000, 0)
    scaled = np.sqrt(w.astype(np.float64)) * out.real
    assert abs(scaled.var() - 1.0) <= 0.05
    assert abs((np.sqrt(w.astype(np.float64)) * out.imag).var() - 1.0) <= 0.05


# ---- the C entry point, without a device ------------------------------------------------------------
def test_entry_point_refuses_before_any_hip_call():
    from katsdpimager_amd import _lib
    fn = _lib.lib().kimg_spectral_filter
    # host addresses far apart: nothing dereferences them
    ptr = dict(vis_in=0x10000000, weights_in=0x20000000, vis_out=0x30000000, weights_out=0x40000000,
               counts=0x50000000)

    def call(coeff=HANNING, length=None, offset=1, step=1, min_sum=0.5, C_in=16, C_out=16, plane=8,
             vip=8, wip=8, vop=8, wop=8, **pointers):
        p = {k: ctypes.c_void_p(v) for k, v in ptr.items()}
        p.update({k: (None if v is None else ctypes.c_void_p(v)) for k, v in pointers.items()})
        c = None
        if coeff is not None:
            keep = np.ascontiguousarray(coeff, np.float64)
            c = keep.ctypes.data_as(ctypes.c_void_p)
        if length is None:
            length = len(coeff)
        return fn(p['vis_in'], vip, p['weights_in'], wip, C_in, p['vis_out'], vop, p['weights_out'], wop,
                  C_out, plane, c, length, offset, step, min_sum, p['counts'], None)
    assert call(plane=0, vip=0, wip=0, vop=0, wop=0) == 0       # the checks pass; nothing to do
    for null in ptr:
        assert call(**{null: None}) == EINVAL
    assert call(coeff=None, length=3) == EINVAL
    assert call(length=0) == EINVAL
    assert call(step=0) == EINVAL
    assert call(offset=-1) == EINVAL
    assert call(offset=3) == EINVAL
    assert call(coeff=(0.25, -0.5, 0.25)) == EINVAL
    assert call(coeff=(0.25, 0.5, np.nan)) == EINVAL
    assert call(coeff=(np.inf, 0.5, 0.25)) == EINVAL
    for bad in (0.0, -1.0, np.nan, np.inf):
        assert call(min_sum=bad) == EINVAL
    assert call(C_out=0) == EINVAL
    assert call(C_out=17) == EINVAL
    assert call(coeff=np.ones(4), offset=0, step=4, C_in=16, C_out=5) == EINVAL
    assert call(coeff=np.ones(4), offset=0, step=4, C_in=16, C_out=4, plane=0, vip=0, wip=0, vop=0,
                wop=0) == 0
    assert call(plane=-1) == EINVAL
    for pitch in ('vip', 'wip', 'vop', 'wop'):
        assert call(**{pitch: 7}) == EINVAL
    # an output that starts inside an input (vis_in: 15 * 8 + 8 complex64 = 1024 bytes)
    assert call(vis_out=ptr['vis_in']) == EINVAL
    assert call(weights_out=ptr['vis_in'] + 1016) == EINVAL
    assert call(weights_out=ptr['weights_in'] + 508) == EINVAL
    assert call(vis_out=ptr['weights_in']) == EINVAL
    # beyond what the kernels are made for
    assert call(coeff=np.ones(73), offset=4, step=64, C_in=64, C_out=1) == EUNSUPPORTED
    assert call(coeff=np.ones(65), offset=0, step=65, C_in=65, C_out=1) == EUNSUPPORTED
    huge = (0x7fffffff * 256) + 1
    assert call(plane=huge, vip=huge, wip=huge, vop=huge, wop=huge) == EUNSUPPORTED
    assert call(coeff=np.ones(72), offset=4, step=64, C_in=64, C_out=1, plane=0, vip=0, wip=0, vop=0,
                wop=0) == 0


# ---- build and ABI surface --------------------------------------------------------------------------
def test_symbol_is_declared_exported_and_prototyped():
    from katsdpimager_amd import _lib, build
    assert 'spectral.hip' in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, 'spectral.hip'))
    assert 'kimg_spectral_filter' in _lib.PROTOTYPES
    assert _lib.lib().kimg_spectral_filter is not None
    header = open(os.path.join(os.path.dirname(build.HERE), 'include', 'kimg.h')).read()
    assert re.search(r'^int kimg_spectral_filter\(', header, re.M)
    defines = dict(re.findall(r'^#define (KIMG_SPECTRAL_MAX_\w+) (\d+)$', header, re.M))
    assert int(defines['KIMG_SPECTRAL_MAX_TAPS']) == spectral.MAX_TAPS == 9
    assert int(defines['KIMG_SPECTRAL_MAX_BIN']) == spectral.MAX_BIN == 64
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


def _dataset(rows=50, C=6):
    rng = np.random.default_rng(2)
    vis = (rng.normal(size=(rows, C, 1)) + 1j * rng.normal(size=(rows, C, 1))).astype(np.complex64)
    return loader.LoaderArrays(rng.normal(size=(rows, 3)).astype(np.float32), vis,
                               np.ones((rows, C, 1), np.float32), np.arange(rows) % 7,
                               1.4e9 + 1e6 * np.arange(C), [0])


def test_loader_refuses_a_collector_of_another_channel_count_before_any_add():
    ident = np.identity(1, np.complex64)
    for channels, params in ((6, SpectralParameters.hanning(bin=2)), (3, SpectralParameters.hanning()),
                             (2, SpectralParameters.average(4))):
        rec = _Recorder(channels)
        with pytest.raises(ValueError):
            loader.preprocess_visibilities(_dataset(), rec, 0, 6, (ident, None), spectral=params)
        assert not any(call[0] == 'add' for call in rec.calls)
    rec = _Recorder(1)
    with pytest.raises(ValueError):         # fewer channels than the bin
        loader.preprocess_visibilities(_dataset(), rec, 0, 3, (ident, None),
                                       spectral=SpectralParameters.average(4))
    assert not rec.calls


def test_loader_refuses_averaging_with_a_continuum_centre():
    from katsdpimager_amd import continuum
    ident = np.identity(1, np.complex64)
    rec = _Recorder(3)
    with pytest.raises(ValueError):
        loader.preprocess_visibilities(
            _dataset(), rec, 0, 6, (ident, None), spectral=SpectralParameters.hanning(bin=2),
            continuum=continuum.UVContSubParameters(0, fit_mask=np.ones(3)),
            continuum_centre=(0.01, 0.02))
    assert not any(call[0] == 'add' for call in rec.calls)
