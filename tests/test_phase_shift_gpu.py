"""Phase-centre shift on the device (csrc/phaseshift.hip through phaseshift.PhaseShift and the C entry
point) against the numpy twin (phaseshift.phase_shift_host_double, tested on its own in
test_phase_shift_host.py), then through the loader into the store and through the driver.

Device against twin, per real component: |dev - t| <= BOUND |v|, t the twin's float64 value, |v| the
modulus of the input visibility, BOUND = 10 * 2^-24 (the issue's cap is 2^-20 = 16 * 2^-24).
With u = 2^-24: the device's sincospif is within 4 ulp (the OpenCL bound its math library is held
to), an ulp of a value below 1 being at most u, so 4 u on each of sin and cos; the first-order
correction by the float32 remainder of the angle adds one rounding, u, to each (what it neglects,
delta^2 / 2 <= 5e-15, and the float64 error of the turn count, 2 pi * 4 * 2^-53 per turn = 1.4e-11
at 5000 turns, are nothing); |re| e + |im| e <= sqrt(2) |v| e makes 7.1 u |v|; the two products round to
u (|re c| + |im s|) <= u |v| and the sum to u |v|: 9.1 u |v|.  Float32 phase arithmetic on these
inputs (1000 turns and more) is wrong by 1e-4 |v| and fails by three orders."""
import ctypes

import numpy as np
import pytest

import golden_inputs as gi
from helpers import context_queue, kernel_taper, make_params, relerr, tapered_relerr, SENTINELS

pytestmark = pytest.mark.gpu

EINVAL = -10001
BOUND = 10.0 * 2.0 ** -24
assert BOUND <= 2.0 ** -20

O = (0.93, -0.52)
T = (0.93 + 0.031, -0.52 + 0.021)       # about 2 degrees away: delay 0.034, 1200 turns at 8 km
SHAPES = [(1, 1), (5, 4), (33, 2), (7, 3)]
ROWS = [1, 63, 64, 65, 257, 4003]
#: bands past 64 channels and past 1024, at a partial second wave and a second workgroup
LONG_SHAPES = [(65, 2), (1025, 1)]
LONG_ROWS = [65, 257]


def _inputs(C, N, Q, seed):
    rng = np.random.default_rng(seed)
    uvw = rng.uniform(-1.0, 1.0, (N, 3))
    uvw *= (8000.0 * rng.uniform(0.01, 1.0, N) / np.linalg.norm(uvw, axis=1))[:, None]
    if N >= 63:
        uvw[11] = [6400.0, 4200.0, -2200.0]         # (a long baseline along the shift, for certain)
    uvw = uvw.astype(np.float32)
    vis = ((rng.normal(size=(C, N, Q)) + 1j * rng.normal(size=(C, N, Q))) * 3.0).astype(np.complex64)
    inv_wl = (1.4e9 + 1.0e6 * np.cumsum(rng.uniform(0.2, 1.7, C))) / 299792458.0
    if N >= 63:
        uvw[5, 1] = np.nan
        uvw[40, 2] = -np.inf
        vis[C // 2, 20, Q - 1] = complex(np.nan, 1.0)
        vis[0, 33, 0] = complex(-2.0, np.inf)
    return vis, uvw, inv_wl


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_against_twin(got, got_uvw, vis, uvw, inv_wl, params):
    from katsdpimager_amd import phaseshift
    want, want_uvw = phaseshift.phase_shift_host_double(vis, uvw, inv_wl, params)
    bad_row = ~np.isfinite(uvw).all(axis=1)
    bad = ~(np.isfinite(vis.real) & np.isfinite(vis.imag)) | bad_row[None, :, None]
    modulus = np.abs(vis.astype(np.complex128))
    worst = 0.0
    for part in ('real', 'imag'):
        d = getattr(got, part).astype(np.float64)
        # a non-finite input makes both parts of its own sample non-finite, and nothing else
        assert np.array_equal(~np.isfinite(d), bad)
        with np.errstate(invalid='ignore'):
            err = np.abs(d - getattr(want, part))[~bad]
        limit = BOUND * modulus[~bad]
        if err.size:
            worst = max(worst, float((err / modulus[~bad]).max()))
        assert (err <= limit).all(), 'worst error {:.3g} |v| against {:.3g}'.format(worst, BOUND)
    if got_uvw is not None:
        assert np.array_equal(~np.isfinite(got_uvw), np.repeat(bad_row[:, None], 3, axis=1))
        good = ~bad_row
        norm = np.linalg.norm(uvw[good].astype(np.float64), axis=1)[:, None]
        err = np.abs(got_uvw[good].astype(np.float64) - want_uvw[good])
        assert (err <= 2.0 ** -24 * np.abs(want_uvw[good]) + 1e-12 * norm).all()
    return worst


class _Embedded:
    """A host array inside a flat device buffer of sentinels, `lead` elements from its start."""

    def __init__(self, ctx, q, inner, lead, tail):
        from katsdpimager_amd import accel
        self.inner_shape, self.lead = inner.shape, lead
        self.host = np.full(lead + inner.size + tail, SENTINELS[inner.dtype], inner.dtype)
        self.host[lead:lead + inner.size] = inner.reshape(-1)
        self.dev = accel.DeviceArray(ctx, self.host.shape, inner.dtype)
        self.dev.set(q, self.host)
        self.ptr = self.dev.ptr + lead * inner.dtype.itemsize

    def get(self, q, written=True):
        out = self.dev.get(q)
        n = int(np.prod(self.inner_shape))
        keep = np.ones(len(out), bool)
        if written:
            keep[self.lead:self.lead + n] = False
        assert np.array_equal(out[keep].view(np.uint8), self.host[keep].view(np.uint8)), 'sentinels changed'
        return out[self.lead:self.lead + n].reshape(self.inner_shape)


@pytest.mark.parametrize('C,Q', SHAPES)
def test_device_against_twin(C, Q):
    _device_against_twin(C, Q, ROWS)


@pytest.mark.parametrize('C,Q', LONG_SHAPES)
def test_device_against_twin_on_long_bands(C, Q):
    _device_against_twin(C, Q, LONG_ROWS)


def _device_against_twin(C, Q, rows):
    from katsdpimager_amd import accel, phaseshift
    from katsdpimager_amd._lib import lib
    ctx, q = context_queue()
    side = ctx.create_command_queue()
    params = phaseshift.PhaseShiftParameters(O, T)
    template = phaseshift.PhaseShiftTemplate(ctx, params)
    p12 = params.params12()
    worst = 0.0
    for i, N in enumerate(rows):
        vis, uvw, inv_wl = _inputs(C, N, Q, 100 * C + i)
        if N >= 63:
            turns = np.abs(inv_wl[:, None] * (uvw[[11]].astype(np.float64) @ params.delay)[None])
            assert turns.max() >= 1000
        # the C entry point: a padded channel pitch, every array inside sentinels
        pitch = N * Q + 5
        padded = np.full((C, pitch), SENTINELS[vis.dtype], np.complex64)
        padded[:, :N * Q] = vis.reshape(C, N * Q)
        d_vis = _Embedded(ctx, q, padded, 3, 0)
        d_in = _Embedded(ctx, q, uvw, 2, 7)
        d_out = _Embedded(ctx, q, np.zeros((N, 3), np.float32), 5, 4)
        d_inv = accel.DeviceArray(ctx, (C,), np.float64)
        d_inv.set(q, inv_wl)
        p12_copy = p12.copy()
        assert lib().kimg_phase_shift(d_vis.ptr, pitch, C, N, Q, d_in.ptr, d_out.ptr, d_inv.ptr,
                                      p12_copy.ctypes.data_as(ctypes.c_void_p), q.handle) == 0
        p12_copy[:] = np.nan            # (the host array may go once the call has returned)
        out = d_vis.get(q)
        assert np.array_equal(out[:, N * Q:].view(np.uint8), padded[:, N * Q:].view(np.uint8)), 'padding changed'
        got = np.ascontiguousarray(out[:, :N * Q]).reshape(C, N, Q)
        got_uvw = d_out.get(q)
        assert np.array_equal(_bits(d_in.get(q, written=False)), _bits(uvw))
        worst = max(worst, _check_against_twin(got, got_uvw, vis, uvw, inv_wl, params))
        # uvw_out = NULL: the same visibilities, no coordinates written anywhere
        d_vis2 = _Embedded(ctx, q, padded, 1, 2)
        assert lib().kimg_phase_shift(d_vis2.ptr, pitch, C, N, Q, d_in.ptr, None, d_inv.ptr,
                                      p12.ctypes.data_as(ctypes.c_void_p), q.handle) == 0
        assert np.array_equal(_bits(d_vis2.get(q)), _bits(out))
        assert np.array_equal(_bits(d_out.get(q)), _bits(got_uvw))
        d_in.get(q, written=False)
        # the operator: dense arrays, a side stream, twice: the same bits
        op = template.instantiate(side, inv_wl)
        e_uvw = accel.DeviceArray(ctx, uvw.shape, np.float32)
        e_uvw.set(side, uvw)
        for call in (1, 2):
            e_vis = accel.DeviceArray(ctx, vis.shape, np.complex64)
            e_vis.set(side, vis)
            new_uvw = op(e_vis, e_uvw)
            assert np.array_equal(_bits(e_vis.get(side)), _bits(got))
            assert np.array_equal(_bits(new_uvw.get(side)), _bits(got_uvw))
        assert op(e_vis, e_uvw, write_uvw=False) is None
        assert np.array_equal(_bits(e_uvw.get(side)), _bits(uvw))
    print('C = {}, Q = {}: worst error {:.3g} |v| (bound {:.3g})'.format(C, Q, worst, BOUND))


def test_return_codes_on_the_device():
    """The refusals of the contract with real device pointers; nothing is written."""
    from katsdpimager_amd import accel, phaseshift
    from katsdpimager_amd._lib import lib
    ctx, q = context_queue()
    C, N, Q = 4, 100, 2
    vis = accel.DeviceArray(ctx, (C, N, Q), np.complex64)
    host_vis = np.full((C, N, Q), 1 + 2j, np.complex64)
    vis.set(q, host_vis)
    uvw = accel.DeviceArray(ctx, (2 * N, 3), np.float32)
    host_uvw = np.arange(6 * N, dtype=np.float32).reshape(2 * N, 3)
    uvw.set(q, host_uvw)
    inv = accel.DeviceArray(ctx, (C,), np.float64)
    inv.set(q, np.full(C, 4.67))
    params = phaseshift.PhaseShiftParameters(O, T)
    p12 = params.params12()

    def call(C=C, N=N, Q=Q, pitch=N * Q, out=uvw.ptr + N * 12, v=vis.ptr, i=inv.ptr, p=p12):
        return lib().kimg_phase_shift(v, pitch, C, N, Q, uvw.ptr, out, i,
                                      None if p is None else p.ctypes.data_as(ctypes.c_void_p), q.handle)
    assert call(v=None) == EINVAL and call(i=None) == EINVAL and call(p=None) == EINVAL
    assert call(C=0) == EINVAL and call(Q=0) == EINVAL and call(N=-1) == EINVAL
    assert call(pitch=N * Q - 1) == EINVAL
    assert call(out=uvw.ptr) == EINVAL and call(out=uvw.ptr + N * 12 - 4) == EINVAL
    assert call(N=0, pitch=0) == 0
    assert np.array_equal(_bits(vis.get(q)), _bits(host_vis))
    assert np.array_equal(_bits(uvw.get(q)), _bits(host_uvw))
    assert call() == 0                              # the two halves of one array adjoin: accepted
    assert not np.array_equal(_bits(vis.get(q)), _bits(host_vis))
    assert np.array_equal(_bits(uvw.get(q)[:N]), _bits(host_uvw[:N]))
    op = phaseshift.PhaseShiftTemplate(ctx, params).instantiate(q, np.full(C, 4.67))
    with pytest.raises(ValueError):
        op(accel.DeviceArray(ctx, (C + 1, N, Q), np.complex64), accel.DeviceArray(ctx, (N, 3), np.float32))
    with pytest.raises(ValueError):
        op(vis, uvw)                                # 2 N rows of coordinates
    with pytest.raises(TypeError):
        op(vis, accel.DeviceArray(ctx, (N, 3), np.float64))


# ---- through the loader into the store, and through the driver --------------------------------------
SOURCE_LM = (90, -70)           # the source, pixels of the 256-pixel field from its centre
SMALL = 128                     # the field imaged around it: the source lies outside it unshifted
LINE_CHANNELS = (6, 10)


def _small_config():
    c = dict(gi.E2E_CONFIGS['degrid'])
    c['pixels'] = SMALL
    c['image_size'] = c['pixel_size'] * SMALL
    c['cell_size'] = c['wavelength'] / c['image_size']
    return c


def _band_arrays():
    """16 channels of 600 rows around O: a 1 Jy source at SOURCE_LM whose flux slopes across the band
    (differently for every row), plus 0.4 Jy more in the line channels; w halved so that the shifted
    w stays inside the W range.  (uvw [R][3], baseline [R], vis [R][C][1], weights, frequencies,
    the source's (ra, dec))"""
    from katsdpimager_amd import continuum, phaseshift
    c = gi.E2E_CONFIGS['degrid']
    C, R = 16, 600
    rng = np.random.default_rng(31)
    uvw = gi.e2e_raw(c)[0][:R].copy()
    uvw[:, 2] *= 0.5
    baseline = np.arange(R) // 30
    freq = 299792458.0 / c['wavelength'] + 1.0e6 * (np.arange(C) - 7)
    l, m = SOURCE_LM[0] * c['pixel_size'], SOURCE_LM[1] * c['pixel_size']
    source = phaseshift.offset_to_radec(O, l, m)
    n1 = -(l * l + m * m) / (1.0 + np.sqrt(1.0 - l * l - m * m))
    turns = (freq / 299792458.0)[None, :] * (uvw.astype(np.float64) @ np.array([l, m, n1]))[:, None]
    x = continuum.legendre_basis(1, C)[1]
    flux = 1.0 + (0.2 * np.cos(0.7 * np.arange(R)))[:, None] * x[None, :]
    flux[:, LINE_CHANNELS[0]:LINE_CHANNELS[1]] += 0.4
    vis = (flux * np.exp(-2j * np.pi * (turns - np.rint(turns)))).astype(np.complex64)[:, :, None]
    weights = rng.uniform(0.5, 1.5, (R, C, 1)).astype(np.float32)
    weights[rng.random((R, C, 1)) < 0.05] = 0.0
    return uvw, baseline, vis, weights, freq, source


@pytest.fixture(scope='module')
def band():
    from katsdpimager_amd import accel, continuum, loader, phaseshift, preprocess
    ctx, q = context_queue()
    c = _small_config()
    ip, gp, ap = make_params(c)
    uvw, baseline, vis, weights, freq, source = _band_arrays()
    C = vis.shape[1]
    ident = np.identity(1, np.complex64)
    inv_wl = phaseshift.inverse_wavelengths(freq)
    contsub = continuum.UVContSubParameters(1, line_ranges=[LINE_CHANNELS], frequencies=freq)

    def store(coords, v, w, **kwargs):
        ds = loader.LoaderArrays(coords, v, w, baseline, freq, [0], phase_centre=O,
                                 longest_baseline=c['longest_baseline'])
        coll = preprocess.VisibilityCollectorDevice(q, [ip] * C, [gp] * C, 1024)
        loader.preprocess_visibilities(ds, coll, 0, C, (ident, None), vis_load=C * 250, **kwargs)
        return coll
    # the device's own rotated coordinates (test_device_against_twin vouches for them)
    params = phaseshift.PhaseShiftParameters(O, source)
    d_uvw = accel.DeviceArray(ctx, uvw.shape, np.float32)
    d_uvw.set(q, uvw)
    d_vis = accel.DeviceArray(ctx, (C, len(uvw), 1), np.complex64)
    d_vis.zero(q)
    op = phaseshift.PhaseShiftTemplate(ctx, params).instantiate(q, inv_wl)
    dev_uvw = op(d_vis, d_uvw).get(q)
    by_channel = np.ascontiguousarray(np.swapaxes(vis, 0, 1))
    w_by_channel = np.ascontiguousarray(np.swapaxes(weights, 0, 1))
    t_vis, _ = phaseshift.phase_shift_host(by_channel, uvw, inv_wl, params)
    # the continuum chain: fit on the source, image around O again
    c_there, _ = phaseshift.phase_shift_host(by_channel, uvw, inv_wl, params)
    c_fit, c_weights, c_counts = continuum.uvcontsub_host(c_there, w_by_channel, contsub)
    c_back, _ = phaseshift.phase_shift_host(
        c_fit, uvw, inv_wl, phaseshift.PhaseShiftParameters(O, O, from_centre=source))
    back = lambda a: np.ascontiguousarray(np.swapaxes(a, 0, 1))     # noqa: E731
    return dict(
        c=c, C=C, source=source,
        device=store(uvw, vis, weights, phase_centre=source),
        twin=store(dev_uvw, back(t_vis), weights),
        twin_abs=store(dev_uvw, back(np.abs(t_vis).astype(np.complex64)), weights),
        chain=store(uvw, vis, weights, continuum=contsub, continuum_centre=source),
        chain_twin=store(uvw, back(c_back), back(c_weights)),
        chain_abs=store(uvw, back(np.abs(c_there).astype(np.complex64)), back(c_weights)),
        chain_counts=c_counts)


def _read(coll, channel, w_slice):
    pieces = [p.copy() for p in coll.reader().iter_slice(channel, w_slice, None)]
    return np.rec.array(np.hstack(pieces)) if pieces else np.rec.recarray(0, coll.store_dtype)


def _same_store(dev, twin, scale, C, per_sample):
    """Same records and coordinates; every stored visibility, a weighted sum of samples, within
    per_sample * sum w |v| (the third store holds that sum) plus 2^-22 of the slice's largest for
    the float32 sums themselves."""
    assert dev.num_input == twin.num_input and dev.num_output == twin.num_output
    records = 0
    for channel in range(C):
        for s in range(dev.reader().num_w_slices(channel)):
            a, b, m = _read(dev, channel, s), _read(twin, channel, s), _read(scale, channel, s)
            assert len(a) == len(b) == len(m)
            records += len(a)
            if not len(a):
                continue
            np.testing.assert_array_equal(a.uv, b.uv)
            np.testing.assert_array_equal(a.sub_uv, b.sub_uv)
            np.testing.assert_array_equal(a.w_plane, b.w_plane)
            np.testing.assert_array_equal(np.asarray(a.weights), np.asarray(b.weights))
            np.testing.assert_array_equal(np.asarray(m.weights), np.asarray(b.weights))
            diff = np.asarray(a.vis).astype(np.complex128) - np.asarray(b.vis)
            weighted = np.asarray(m.vis).real.astype(np.float64)
            limit = per_sample * weighted + 2.0 ** -22 * weighted.max()
            assert (np.abs(diff.real) <= limit).all() and (np.abs(diff.imag) <= limit).all()
    assert records > 1000


def test_stream_matches_twin_shifted_store(band):
    assert band['device'].phase_centre == band['source']
    assert not hasattr(band['twin'], 'phase_centre')
    # BOUND on the device, 2^-24 for the twin's own rounding to complex64
    _same_store(band['device'], band['twin'], band['twin_abs'], band['C'], BOUND + 2.0 ** -24)


def test_stream_with_the_continuum_fit_on_the_source(band):
    """O -> S, the fit, S -> O against the twins' chain.  Per sample, in units of the largest
    unsubtracted |v| of its channels: the first shift leaves BOUND + 2^-24 (the twin's rounding)
    between device and twin; the fit, float64 on both sides (test_uvcontsub_gpu.py), subtracts a
    weighted mean and slope of those errors, a linear map whose absolute row sum is at most 2 (5 / 3
    for a line across evenly weighted channels, at the band's edge), so 3 (BOUND + 2^-24) after it,
    plus 2 * 2^-24 for the two roundings of the results; the second shift adds BOUND + 2^-24 of a
    residual that is smaller than the input.  The channels of a sample differ in |v| by at most 2
    (flux 0.8 to 1.6), and the store's scale is the channel's own: twice 4 BOUND + 6 * 2^-24."""
    chain = band['chain']
    assert chain.phase_centre == O
    assert chain.continuum_counts == band['chain_counts'] and band['chain_counts'][0] > 500
    _same_store(chain, band['chain_twin'], band['chain_abs'], band['C'], 2 * (4 * BOUND + 6 * 2.0 ** -24))


def test_driver_images_a_small_field_around_the_new_centre(band):
    from katsdpimager_amd import frontend, imaging, parameters, weight
    ctx, q = context_queue()
    c = band['c']
    ip, gp, ap = make_params(c)
    wp = parameters.WeightParameters(weight.WeightType(c['weight_type']), c['robustness'])
    # one component: the dirty image's peak, and a residual that is the dirty image less one PSF
    cp = parameters.CleanParameters(1, c['loop_gain'], c['major_gain'], c['threshold'],
                                    c['mode'], c['psf_cutoff'], c['psf_limit'], c['border'])
    im = imaging.ImagingTemplate(ctx, ap, ip.fixed, wp, gp.fixed, cp).instantiate(
        q, ip, gp, c['vis_block'], 0, 1)
    im.ensure_all_bound()
    images = {}
    for name in ('device', 'twin'):
        stats = frontend.process_channel(band[name].reader(), 3, im, ip, gp, cp, wp.weight_type,
                                         c['vis_block'], 1, c['degrid'])
        assert stats is not None and stats['major'] == 1 and len(stats['peaks']) == 1
        model = im.get_buffer('model')[0].copy()
        assert np.count_nonzero(model) == 1
        y, x = np.unravel_index(np.argmax(np.abs(model)), model.shape)
        assert (y, x) == (SMALL // 2, SMALL // 2)
        assert 0.5 < stats['peaks'][0] < 1.5
        images[name] = (im.get_buffer('dirty')[0].copy(), model, stats['peaks'][0])
    (dirty_a, model_a, peak_a), (dirty_b, model_b, peak_b) = images['device'], images['twin']
    # the residual is the dirty image less one PSF; norm-wise before the division by the taper, as
    # images are compared everywhere here (helpers.tapered_relerr)
    assert tapered_relerr(dirty_a, dirty_b, kernel_taper(c)) <= 1e-5
    assert relerr(model_a, model_b) <= 1e-5
    assert abs(peak_a - peak_b) <= 1e-5 * peak_b
