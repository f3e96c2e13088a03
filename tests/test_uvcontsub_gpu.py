"""UV-plane continuum subtraction on the device (csrc/contsub.hip through continuum.UVContSub) against
the numpy twin (continuum.uvcontsub_host, tested on its own in test_uvcontsub_host.py), then through
the loader into the store and through the driver.

Device against twin, per real component: |dev - t| <= 2^-24 |t| + 1e-9 S, t the twin's value BEFORE
its final rounding to float32 and S the sample's largest |v|.  The first term is the one rounding
the contract allows; the second covers float64 arithmetic in another order, about
K^2 cond(A) 2^-53 S = 7e-13 S at the conditioning these inputs are held to (cond(A) <= 1e3,
asserted below) -- three orders inside the bound, while any float32 step in the fit lands near
1e-7 S and fails."""
import numpy as np
import pytest

import band_cases as bands
import golden_inputs as gi
from helpers import context_queue, make_params, SENTINELS

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -10001, -10002

SHAPES = [
    (24, 3, [1] * 9 + [0] * 6 + [1] * 9),
    (5, 3, [1] * 5),
    (16, 1, [1] * 6 + [0] * 4 + [1] * 6),
    (7, 2, [1, 1, 0, 0, 0, 1, 1]),
    (1, 0, [1]),
]
#: (N, Q): one element, partial / whole / whole + 1 waves, partial workgroups
PLANES = [(1, 1), (63, 1), (64, 1), (65, 1), (1000, 1), (1000, 2), (1000 * 4 + 3, 1)]


def _inputs(C, order, mask, N, Q, seed, pool=None):
    """Weights U(0.5, 2) with 20 % zeros, and, where the plane has room, hand-made samples: one that
    cannot be fitted (m = K - 1), one with m == K exactly on well-spread channels (the others
    knocked out by a zero weight, a negative weight or a NaN in turn), a NaN and a negative weight
    in a fit channel, a NaN in a line channel.  ``pool``: the fit channels that the surviving
    channels of the first two, and the NaN and the negative weight, are taken from (all of them by
    default)."""
    rng = np.random.default_rng(seed)
    K = order + 1
    vis = ((rng.normal(size=(C, N, Q)) + 1j * rng.normal(size=(C, N, Q))) * 3.0).astype(np.complex64)
    weights = rng.uniform(0.5, 2.0, (C, N, Q)).astype(np.float32)
    weights[rng.random((C, N, Q)) < 0.2] = 0.0
    fit = np.flatnonzero(mask)
    line = np.flatnonzero(np.asarray(mask) == 0)
    pool = fit if pool is None else np.asarray(pool)
    v2, w2 = vis.reshape(C, N * Q), weights.reshape(C, N * Q)       # (views)

    def keep_only(j, channels):
        w2[fit, j] = rng.uniform(0.5, 2.0, len(fit))
        for i, c in enumerate(np.setdiff1d(fit, channels)):
            if i % 3 == 0:
                w2[c, j] = 0.0
            elif i % 3 == 1:
                w2[c, j] = -1.5
            else:
                v2[c, j] = complex(np.nan, 2.0) if i % 2 else complex(-1.0, np.inf)
    if N * Q >= 63:
        spread = pool[np.round(np.linspace(0, len(pool) - 1, K)).astype(int)]
        keep_only(3, spread[:K - 1])            # m = K - 1: flagged
        keep_only(5, spread)                    # m == K
        keep_only(40, fit)                      # every fit channel usable ...
        keep_only(41, fit)
        v2[pool[len(pool) // 2], 40] = np.nan   # ... but one NaN
        w2[pool[0], 41] = -0.75                 # ... but one negative weight
        if len(line):
            w2[:, 42] = rng.uniform(0.5, 2.0, C)
            v2[line[0], 42] = complex(3.0, np.nan)
    return vis, weights


def _cond(weights, vis, C, order, mask, frequencies=None):
    """The largest cond(A) over the samples that are fitted."""
    from katsdpimager_amd.continuum import legendre_basis
    B = legendre_basis(order, C, frequencies)
    usable = (np.asarray(mask, bool)[:, None, None] & (weights > 0)
              & np.isfinite(vis.real) & np.isfinite(vis.imag))
    w = np.where(usable, weights.astype(np.float64), 0.0)
    A = np.einsum('cnq,kc,lc->nqkl', w, B, B)
    fitted = usable.sum(axis=0) >= order + 1
    return float(np.linalg.cond(A[fitted]).max()) if fitted.any() else 1.0


class _PaddedBlock:
    """[C][N][Q] inside a [C][pitch] device buffer of sentinels."""

    def __init__(self, ctx, q, inner, pad):
        from katsdpimager_amd import accel
        C, N, Q = inner.shape
        self.plane = N * Q
        self.host = np.full((C, self.plane + pad), SENTINELS[inner.dtype], inner.dtype)
        self.host[:, :self.plane] = inner.reshape(C, self.plane)
        self.whole = accel.DeviceArray(ctx, self.host.shape, inner.dtype)
        self.whole.set(q, self.host)
        view = self.whole.tensor[:, :self.plane].unflatten(1, (N, Q))
        self.array = accel.DeviceArray(ctx, inner.shape, inner.dtype, tensor=view)
        self.shape = inner.shape

    def get(self, q):
        out = self.whole.get(q)
        assert np.array_equal(out[:, self.plane:].view(np.uint8),
                              self.host[:, self.plane:].view(np.uint8)), 'padding changed'
        return np.ascontiguousarray(out[:, :self.plane]).reshape(self.shape)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_against_twin(got_vis, got_weights, vis, weights, params):
    from katsdpimager_amd import continuum
    want, want_weights, fitted = continuum.uvcontsub_host_double(vis, weights, params)
    finite = np.isfinite(vis.real) & np.isfinite(vis.imag)
    S = np.where(finite, np.abs(vis.astype(np.complex128)), 0.0).max(axis=0)
    for part in ('real', 'imag'):
        t = getattr(want, part)[:, fitted]
        d = getattr(got_vis, part)[:, fitted].astype(np.float64)
        nan = np.isnan(t)
        assert np.array_equal(np.isnan(d), nan)
        inf = np.isinf(t)
        assert np.array_equal(d[inf], t[inf])
        ok = ~(nan | inf)
        with np.errstate(invalid='ignore'):
            err = np.abs(d - t)[ok]
        bound = (2.0 ** -24 * np.abs(t) + 1e-9 * S[fitted][None])[ok]
        assert (err <= bound).all(), 'worst excess {:.3g}'.format(float((err - bound).max()))
    # samples that could not be fitted: visibilities untouched, weights exactly 0; the others'
    # weights bit for bit the input's
    assert np.array_equal(_bits(got_vis[:, ~fitted]), _bits(vis[:, ~fitted]))
    assert np.array_equal(_bits(got_weights), _bits(want_weights))
    assert (got_weights[:, ~fitted] == 0).all() and not np.signbit(got_weights[:, ~fitted]).any()
    n = int(fitted.sum())
    return n, fitted.size - n


@pytest.mark.parametrize('C,order,mask', SHAPES)
def test_device_against_twin(C, order, mask):
    from katsdpimager_amd import continuum
    ctx, q = context_queue()
    side = ctx.create_command_queue()
    params = continuum.UVContSubParameters(order, fit_mask=mask)
    template = continuum.UVContSubTemplate(ctx, params)
    for i, (N, Q) in enumerate(PLANES):
        vis, weights = _inputs(C, order, mask, N, Q, 1000 * C + i)
        assert _cond(weights, vis, C, order, mask) <= 1e3
        op = template.instantiate(q, C)
        assert op.counts() == (0, 0)
        # padded channel pitches, different for the two arrays
        d_vis = _PaddedBlock(ctx, q, vis, 5)
        d_weights = _PaddedBlock(ctx, q, weights, 11)
        op(d_vis.array, d_weights.array)
        got_vis, got_weights = d_vis.get(q), d_weights.get(q)
        counts = _check_against_twin(got_vis, got_weights, vis, weights, params)
        assert sum(counts) == N * Q
        if N * Q >= 63:
            assert counts[1] >= 1 and counts[0] >= 1
        assert op.counts() == counts
        # dense arrays, a side stream, the same operator parameters: the same bits, and the counts
        # of an operator add up over its calls
        from katsdpimager_amd import accel
        op2 = template.instantiate(side, C)
        for call in (1, 2):
            e_vis = accel.DeviceArray(ctx, vis.shape, np.complex64)
            e_weights = accel.DeviceArray(ctx, weights.shape, np.float32)
            e_vis.set(side, vis)
            e_weights.set(side, weights)
            op2(e_vis, e_weights)
            assert np.array_equal(_bits(e_vis.get(side)), _bits(got_vis))
            assert np.array_equal(_bits(e_weights.get(side)), _bits(got_weights))
            assert op2.counts() == (call * counts[0], call * counts[1])
        op2.reset_counts()
        assert op2.counts() == (0, 0)


# ---- bands longer than one word of the fit mask (band_cases.py) --------------------------------------
def seam_case(C, order, mask):
    """(pool, frequencies) of a long-band case.  ``pool``: the fit channels outside word 0 of the mask
    (all fit channels where fewer than K lie there), from which the hand-made samples of _inputs take
    their surviving channels.  ``frequencies``: the step into a channel of the pool is 1 MHz, into any
    other channel 1/256 MHz, so that the pool lies evenly over x in [-1, 1] whatever the mask: with a
    mask that confines the fit channels to the last 33 of 1025, evenly spaced channels would put them
    on x in [0.94, 1], where cond(A) of an order-1 fit is already 1e4 by geometry alone and the bound
    of this file does not apply."""
    fit = np.flatnonzero(mask)
    pool = fit[fit >= bands.WORD]
    if len(pool) < order + 1:
        pool = fit
    step = np.full(C, 1.0 / 256.0)
    step[pool] = 1.0
    return pool, 1.4e9 + 1.0e6 * np.cumsum(step)


def seam_inputs(C, order, mask, N, Q, seed):
    """(vis, weights, params, pool) of a long-band case."""
    from katsdpimager_amd import continuum
    pool, frequencies = seam_case(C, order, mask)
    params = continuum.UVContSubParameters(order, fit_mask=mask, frequencies=frequencies)
    vis, weights = _inputs(C, order, mask, N, Q, seed, pool=pool)
    return vis, weights, params, pool


def _run_padded(ctx, q, params, vis, weights):
    """The operator on padded channel pitches, different for the two arrays (the padding is checked
    to come back unchanged): (vis, weights, counts)."""
    from katsdpimager_amd import continuum
    op = continuum.UVContSubTemplate(ctx, params).instantiate(q, vis.shape[0])
    d_vis = _PaddedBlock(ctx, q, vis, 5)
    d_weights = _PaddedBlock(ctx, q, weights, 11)
    op(d_vis.array, d_weights.array)
    return d_vis.get(q), d_weights.get(q), op.counts()


@pytest.mark.parametrize('order', [0, 1, 2, 3])
@pytest.mark.parametrize('C', bands.CHANNELS)
def test_device_against_twin_past_one_mask_word(C, order):
    """Every mask of band_cases that leaves order + 1 fit channels, on both planes: the bound and the
    condition of test_device_against_twin, unchanged.  (A different summation order over C terms
    costs about C 2^-53 cond(A) S, 1e-10 S at 1025 channels and cond(A) = 1e3.)"""
    ctx, q = context_queue()
    ran = 0
    for i, (name, mask) in enumerate(bands.masks(C, least=order + 1)):
        for k, (N, Q) in enumerate(bands.PLANES):
            vis, weights, params, pool = seam_inputs(C, order, mask, N, Q, 7000 * C + 10 * i + k)
            assert _cond(weights, vis, C, order, mask, params.frequencies) <= 1e3, (name, N, Q)
            got_vis, got_weights, counts = _run_padded(ctx, q, params, vis, weights)
            try:
                want = _check_against_twin(got_vis, got_weights, vis, weights, params)
            except AssertionError as e:
                raise AssertionError('{} at {}'.format(e, (C, order, name, N, Q))) from None
            assert counts == want and sum(counts) == N * Q
            assert counts[0] >= 1 and counts[1] >= 1
            ran += 1
    assert ran == 2 * len(bands.masks(C, least=order + 1)) and ran >= 6


def test_one_launch_at_the_longest_band():
    """MAX_CHANNELS channels, 512 words of mask by value in the kernel arguments, order 3: the only
    line channels are 8191, 8192 and two of the last word."""
    from katsdpimager_amd import continuum
    ctx, q = context_queue()
    C, N, Q, order = continuum.MAX_CHANNELS, 65, 2, 3
    assert C == 16384
    mask = bands.limit_mask(C)
    vis, weights, params, pool = seam_inputs(C, order, mask, N, Q, 16384)
    assert _cond(weights, vis, C, order, mask, params.frequencies) <= 1e3
    got_vis, got_weights, counts = _run_padded(ctx, q, params, vis, weights)
    want = _check_against_twin(got_vis, got_weights, vis, weights, params)
    assert counts == want and counts[0] >= 1 and counts[1] >= 1 and sum(counts) == N * Q


def test_refusals_on_the_device():
    """The return codes of the contract with real device pointers; nothing is written."""
    from katsdpimager_amd import accel, continuum
    from katsdpimager_amd._lib import lib
    import ctypes
    ctx, q = context_queue()
    C, N = 8, 100
    vis = accel.DeviceArray(ctx, (C, N, 1), np.complex64)
    weights = accel.DeviceArray(ctx, (C, N, 1), np.float32)
    vis.zero(q)
    host_w = np.full((C, N, 1), 2.0, np.float32)
    weights.set(q, host_w)
    basis = accel.DeviceArray(ctx, (4, C), np.float64)
    basis.set(q, continuum.legendre_basis(3, C))
    counts = accel.DeviceArray(ctx, (2,), np.int64)
    counts.zero(q)

    def call(num_channels, order, mask, vp=N, wp=N):
        m = np.asarray(mask, np.uint8)
        return lib().kimg_uvcontsub(vis.ptr, vp, weights.ptr, wp, num_channels, N,
                                    m.ctypes.data_as(ctypes.c_void_p), basis.ptr, order, counts.ptr,
                                    q.handle)
    full = np.ones(C, np.uint8)
    assert call(C, 4, full) == EINVAL
    assert call(C, -1, full) == EINVAL
    assert call(0, 0, full) == EINVAL
    assert call(C, 0, np.zeros(C)) == EUNSUPPORTED
    assert call(C, 3, [1, 1, 0, 0, 0, 0, 0, 1]) == EUNSUPPORTED
    assert call(C, 1, full, vp=N - 1) == EINVAL
    assert call(C, 1, full, wp=N - 1) == EINVAL
    with pytest.raises(ValueError):
        continuum.UVContSubTemplate(ctx, continuum.UVContSubParameters(1, fit_mask=full)).instantiate(q, C + 1)
    assert counts.get(q).tolist() == [0, 0]
    assert np.array_equal(weights.get(q), host_w)
    assert call(C, 3, [1, 1, 0, 0, 0, 0, 1, 1]) == 0           # K fit channels exactly: accepted
    assert counts.get(q).tolist() == [N, 0]


# ---- through the loader into the store, and through the driver --------------------------------------
LINE_LM = (20, -33)         # the line source, pixels from the centre
LINE_CHANNELS = (6, 10)


def _band_arrays():
    """16 channels of a few hundred rows: a continuum source at the phase centre whose flux is an
    order-1 polynomial of the channel (a different one for every row), a line source off centre
    in channels 6-9, weights U(0.5, 1.5) with some zeros, three rows with a single usable
    line-free channel.  (uvw [R][3], baseline [R], vis [R][C][1], weights [R][C][1], parameters)"""
    from katsdpimager_amd import continuum
    c = gi.E2E_CONFIGS['degrid']
    C, R = 16, 600
    rng = np.random.default_rng(21)
    uvw = gi.e2e_raw(c)[0][:R]
    baseline = np.arange(R) // 30                   # (e2e_raw: tracks of 30 consecutive rows)
    x = continuum.legendre_basis(1, C)[1]
    amp = 2.0 + 0.3 * np.sin(np.arange(R))
    slope = 0.5 * np.cos(0.7 * np.arange(R))
    vis = amp[:, None] + slope[:, None] * x[None, :] + 0j           # [R][C]
    l, m = LINE_LM[0] * c['pixel_size'], LINE_LM[1] * c['pixel_size']
    n = np.sqrt(1 - l * l - m * m)
    uvw_wl = uvw.astype(np.float64) / c['wavelength']
    line = 0.4 / n * np.exp(-2j * np.pi * (uvw_wl[:, 0] * l + uvw_wl[:, 1] * m + uvw_wl[:, 2] * (n - 1)))
    vis[:, LINE_CHANNELS[0]:LINE_CHANNELS[1]] += line[:, None]
    vis = vis.astype(np.complex64)[:, :, None]
    weights = rng.uniform(0.5, 1.5, (R, C, 1)).astype(np.float32)
    weights[rng.random((R, C, 1)) < 0.05] = 0.0
    for row in (17, 300, 599):
        weights[row, :, 0] = 0.0
        weights[row, 2, 0] = 1.0                    # one usable line-free channel: cannot be fitted
        weights[row, 7, 0] = 1.0                    # (and a line channel, which does not count)
    params = continuum.UVContSubParameters(1, line_ranges=[LINE_CHANNELS])
    return uvw, baseline, vis, weights, params


@pytest.fixture(scope='module')
def band():
    """The stores made of :func:`_band_arrays` with the operator in the stream, of the twin's
    output without it, and of the raw data."""
    from katsdpimager_amd import continuum, loader, preprocess
    ctx, q = context_queue()
    c = gi.E2E_CONFIGS['degrid']
    ip, gp, ap = make_params(c)
    uvw, baseline, vis, weights, params = _band_arrays()
    C = vis.shape[1]
    freq = 1.4e9 + 1e6 * np.arange(C)
    ident = np.identity(1, np.complex64)
    vis_load = C * 250                              # three blocks

    def store(v, w, **kwargs):
        ds = loader.LoaderArrays(uvw, v, w, baseline, freq, [0], longest_baseline=c['longest_baseline'])
        coll = preprocess.VisibilityCollectorDevice(q, [ip] * C, [gp] * C, 1024)
        loader.preprocess_visibilities(ds, coll, 0, C, (ident, None), vis_load=vis_load, **kwargs)
        return coll
    t_vis, t_weights, t_counts = continuum.uvcontsub_host(
        np.ascontiguousarray(np.swapaxes(vis, 0, 1)), np.ascontiguousarray(np.swapaxes(weights, 0, 1)),
        params)
    return dict(
        c=c, C=C, params=params, twin_counts=t_counts,
        device=store(vis, weights, continuum=params),
        twin=store(np.swapaxes(t_vis, 0, 1), np.swapaxes(t_weights, 0, 1)),
        raw=store(vis, weights))


def _read(coll, channel, w_slice):
    pieces = [p.copy() for p in coll.reader().iter_slice(channel, w_slice, None)]
    return np.rec.array(np.hstack(pieces)) if pieces else np.rec.recarray(0, coll.store_dtype)


def test_stream_matches_twin_subtracted_store(band):
    dev, twin = band['device'], band['twin']
    assert band['twin_counts'] == (597, 3)
    assert dev.continuum_counts == band['twin_counts']
    assert not hasattr(twin, 'continuum_counts')
    assert dev.num_input == twin.num_input and dev.num_output == twin.num_output
    records = 0
    for channel in range(band['C']):
        for s in range(dev.reader().num_w_slices(channel)):
            a, b = _read(dev, channel, s), _read(twin, channel, s)
            assert len(a) == len(b)
            records += len(a)
            if not len(a):
                continue
            np.testing.assert_array_equal(a.uv, b.uv)
            np.testing.assert_array_equal(a.sub_uv, b.sub_uv)
            np.testing.assert_array_equal(a.w_plane, b.w_plane)
            np.testing.assert_array_equal(np.asarray(a.weights), np.asarray(b.weights))
            # one ulp per sample from rounding nearly equal doubles, one for the weight multiply,
            # the rest spare
            largest = np.abs(b.vis).max()
            assert np.abs(np.asarray(a.vis) - np.asarray(b.vis)).max() <= 2.0 ** -22 * largest
    assert records > 1000


def test_driver_images_the_line_and_nothing_else(band):
    from katsdpimager_amd import frontend, imaging, parameters, weight
    ctx, q = context_queue()
    c = band['c']
    dev, raw = band['device'], band['raw']
    ip, gp, ap = make_params(c)
    # a line-free channel: what is left of the order-1 continuum at the phase centre is rounding
    S = max(np.abs(_read(raw, ch, s).vis).max() for ch in range(band['C'])
            for s in range(raw.reader().num_w_slices(ch)) if raw.reader().len(ch, s))
    for channel in (0, 5, 12):
        left = max(np.abs(_read(dev, channel, s).vis).max()
                   for s in range(dev.reader().num_w_slices(channel)) if dev.reader().len(channel, s))
        assert left <= 2.0 ** -22 * S
    # a line channel through the driver: one major cycle; the components sit on the line source
    wp = parameters.WeightParameters(weight.WeightType(c['weight_type']), c['robustness'])
    cp = parameters.CleanParameters(c['minor'], c['loop_gain'], c['major_gain'], c['threshold'],
                                    c['mode'], c['psf_cutoff'], c['psf_limit'], c['border'])
    im = imaging.ImagingTemplate(ctx, ap, ip.fixed, wp, gp.fixed, cp).instantiate(
        q, ip, gp, c['vis_block'], 0, c['major'])
    im.ensure_all_bound()
    stats = frontend.process_channel(dev.reader(), 7, im, ip, gp, cp, wp.weight_type, c['vis_block'],
                                     1, c['degrid'])
    assert stats is not None and stats['major'] == 1 and stats['minor'] >= 1
    model = im.get_buffer('model')[0]
    G = c['pixels']
    y, x = np.unravel_index(np.argmax(np.abs(model)), model.shape)
    assert (y, x) == (G // 2 + LINE_LM[1], G // 2 + LINE_LM[0])
    assert model[y, x] > 0 and 0.05 < stats['peaks'][0] < 0.6
