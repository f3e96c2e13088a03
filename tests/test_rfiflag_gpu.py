"""RFI flagging on the device (csrc/rfiflag.hip through rfiflag.RFIFlag) against the numpy twin
(rfiflag.rfiflag_host, tested on its own in test_rfiflag_host.py), then through the loader into the
store next to the other operators.

The contract fixes the order of every float64 sum and the build contracts nothing into fused
multiply-adds, so the device has the twin's bits: flags are compared byte for byte, weights as uint32
patterns, the level as uint64 patterns (NaN in the same places), counts exactly.

The blocks come from rfiflag_cases.inputs: per longest window (1, 2, 16, 32) bands of 1, 2, one less
than, exactly and one more than that window, and 65 channels, at 1, 63, 64, 65 and 1000 rows in
baseline runs of 1 to 150 rows, 1 to 4 polarizations, with time_bin 1, 3 and 64, the three
directions and 0, 2 and 4 level iterations taken in turn; noise with 20 % zero weights, negative
and infinite weights, NaN and Inf visibilities, protected channels of which one is bright, and
spikes, runs, bursts and rows without weight embedded in it."""
import numpy as np
import pytest

import band_cases as bands
import golden_inputs as gi
import rfiflag_cases as cases
from helpers import context_queue, make_params, SENTINELS

pytestmark = pytest.mark.gpu


class _PaddedBlock:
    """[C][N][P] inside a [C][pitch] device buffer of sentinels (test_statwt_gpu._PaddedBlock)."""

    def __init__(self, ctx, q, inner, pad):
        from katsdpimager_amd import accel
        C, N, P = inner.shape
        self.plane = N * P
        self.host = np.full((C, self.plane + pad), SENTINELS[inner.dtype], inner.dtype)
        self.host[:, :self.plane] = inner.reshape(C, self.plane)
        self.whole = accel.DeviceArray(ctx, self.host.shape, inner.dtype)
        self.whole.set(q, self.host)
        view = self.whole.tensor[:, :self.plane].unflatten(1, (N, P))
        self.array = accel.DeviceArray(ctx, inner.shape, inner.dtype, tensor=view)
        self.shape = inner.shape

    def get(self, q):
        out = self.whole.get(q)
        assert np.array_equal(out[:, self.plane:].view(np.uint8),
                              self.host[:, self.plane:].view(np.uint8)), 'padding changed'
        return np.ascontiguousarray(out[:, :self.plane]).reshape(self.shape)


def _run(ctx, q, op, vis, weights, ids):
    """op on padded channel pitches, different for the two arrays: (weights, flags, level) on the
    host, the padding and the visibilities checked to be what they were."""
    d_vis = _PaddedBlock(ctx, q, vis, 5)
    d_weights = _PaddedBlock(ctx, q, weights, 11)
    op(d_vis.array, d_weights.array, ids)
    got = d_weights.get(q)
    assert np.array_equal(d_vis.get(q).view(np.uint32), vis.view(np.uint32)), 'the visibilities changed'
    return got, op.flags.get(q), op.level.get(q)


@pytest.mark.parametrize('max_window', [1, 2, 16, 32])
def test_device_against_twin(max_window):
    from katsdpimager_amd import rfiflag
    ctx, q = context_queue()
    seen = set()
    total = np.zeros(3, np.int64)
    i = 0
    for C in cases.channels(max_window):
        for N in cases.ROWS:
            for P in cases.POLS:
                time_bin = cases.TIME_BINS[i % 3]
                directions = cases.DIRECTIONS[(i // 3) % 3]
                iterations = cases.LEVEL_ITERATIONS[(i // 9) % 3]
                i += 1
                vis, weights, ids, mask = cases.inputs(C, N, P, 1000 * max_window + 10 * N + P + C)
                params = rfiflag.RFIFlagParameters(time_bin, max_window=max_window, directions=directions,
                                                   level_iterations=iterations, fit_mask=mask,
                                                   extend_pols=bool(i % 5))
                want = rfiflag.rfiflag_host(vis, weights, ids, params)
                op = rfiflag.RFIFlagTemplate(ctx, params).instantiate(q, C)
                assert op.counts() == (0, 0, 0) and op.flags is None and op.level is None
                got = _run(ctx, q, op, vis, weights, ids)
                try:
                    cases.assert_same(got + (op.counts(),), want)
                except AssertionError as e:
                    raise AssertionError('{} at {}'.format(e, (C, N, P, params))) from None
                seen |= {('P', P, time_bin), ('d', directions, time_bin), ('i', iterations)}
                total += want[3]
    assert len(seen) == 4 * 3 + 3 * 3 + 3
    # the blocks held something of everything: samples kept, samples flagged, pairs skipped
    assert total.min() > 0


@pytest.mark.parametrize('N,P', bands.PLANES)
@pytest.mark.parametrize('C', [97, 1025])
def test_device_against_twin_past_one_mask_word(C, N, P):
    """Windows of up to 32 samples in both directions over bands of four and of 33 mask words, the
    protected channels those of every mask of band_cases (rfiflag_cases.band_inputs): a bright
    protected channel at the start of word 1, a hot run under a window of 32 across the seam at 64."""
    from katsdpimager_amd import rfiflag
    ctx, q = context_queue()
    total = np.zeros(3, np.int64)
    names = set()
    for i, (name, mask) in enumerate(bands.masks(C)):
        time_bin = cases.TIME_BINS[i % 3]
        vis, weights, ids, mask = cases.band_inputs(C, N, P, 100 * C + 10 * N + i, mask)
        params = rfiflag.RFIFlagParameters(time_bin, max_window=32, directions='both',
                                           level_iterations=cases.LEVEL_ITERATIONS[i % 3], fit_mask=mask,
                                           extend_pols=bool(i % 2))
        want = rfiflag.rfiflag_host(vis, weights, ids, params)
        op = rfiflag.RFIFlagTemplate(ctx, params).instantiate(q, C)
        got = _run(ctx, q, op, vis, weights, ids)
        try:
            cases.assert_same(got + (op.counts(),), want)
        except AssertionError as e:
            raise AssertionError('{} at {}'.format(e, (C, N, P, name, params))) from None
        total += want[3]
        names.add(name)
    assert len(names) == len(bands.MASKS)
    # the blocks held something of everything: samples kept, samples flagged, pairs skipped
    assert total.min() > 0


def test_one_launch_at_the_longest_band():
    """16384 channels, 512 words of mask by value in the kernel arguments: the only protected channels
    are 32, 8191, 8192 and two of the last word; the workspace is the one workspace_bytes states."""
    from katsdpimager_amd import continuum, rfiflag
    ctx, q = context_queue()
    C, N, P = continuum.MAX_CHANNELS, 6, 2
    assert C == 16384
    vis, weights, ids, mask = cases.band_inputs(C, N, P, 16384, bands.limit_mask(C))
    weights[:, 2, 1] = 0.0                          # (a row without weight: time_bin 1 skips it)
    params = rfiflag.RFIFlagParameters(1, max_window=32, directions='both', fit_mask=mask)
    want = rfiflag.rfiflag_host(vis, weights, ids, params)
    assert min(want[3]) > 0
    op = rfiflag.RFIFlagTemplate(ctx, params).instantiate(q, C)
    got = _run(ctx, q, op, vis, weights, ids)
    cases.assert_same(got + (op.counts(),), want)
    assert op._workspace.shape[0] == op.workspace_bytes(C, N, P) == 9 * C * N * P + 24 * N * P


def test_the_longest_window_along_time_in_a_group_that_holds_it():
    """max_window 32 along time with time_bin 64, in a block whose middle baseline has 40 rows that
    start inside one wave and end in the next: 32 rows of one channel at twice the background are
    0.9 levels above the level, under the 1.19 of a window of 16 and over the 0.79 of a window of
    32, so that window and no other has them; the baselines around it are noise."""
    from katsdpimager_amd import rfiflag
    ctx, q = context_queue()
    C, P = 8, 2
    before = cases.inputs(C, 50, P, 5, protect=False)
    vis = np.concatenate((before[0], np.ones((C, 40, P), np.complex64), before[0][:, :30]), axis=1)
    weights = np.concatenate((before[1], np.ones((C, 40, P), np.float32), before[1][:, :30]), axis=1)
    ids = np.concatenate((np.zeros(50, np.int32), np.full(40, 7, np.int32), np.full(30, 2, np.int32)))
    weights[5, 54:86, 1] = 2.0
    results = {}
    for max_window in (16, 32):
        params = rfiflag.RFIFlagParameters(64, max_window=max_window, directions='time', extend_time=None,
                                           extend_pols=False)
        want = rfiflag.rfiflag_host(vis, weights, ids, params)
        op = rfiflag.RFIFlagTemplate(ctx, params).instantiate(q, C)
        got = _run(ctx, q, op, vis, weights, ids)
        cases.assert_same(got + (op.counts(),), want)
        results[max_window] = got[1][:, 50:90]
    assert not results[16].any()
    assert results[32][5, 4:36, 1].all() and results[32].sum() == 32


def test_repeated_calls_and_a_growing_workspace():
    """The same operator on a small block, then, after reset_counts, on a larger one (the workspace
    grows) and on the small one again (it stays): each call has the twin's bits, the counts add up
    over calls and an empty block changes nothing."""
    from katsdpimager_amd import accel, rfiflag
    ctx, q = context_queue()
    C = 24
    small = cases.inputs(C, 65, 2, 77)
    large = cases.inputs(C, 1000, 2, 78)
    assert np.array_equal(small[3], large[3])
    params = rfiflag.RFIFlagParameters(16, fit_mask=small[3])
    op = rfiflag.RFIFlagTemplate(ctx, params).instantiate(q, C)
    total = np.zeros(3, np.int64)
    sizes = []
    for vis, weights, ids, _ in (small, large, small):
        want = rfiflag.rfiflag_host(vis, weights, ids, params)
        got = _run(ctx, q, op, vis, weights, ids)
        total += want[3]
        cases.assert_same(got + (tuple(total),), want[:3] + (op.counts(),))
        sizes.append(op._workspace.shape[0])
        if len(sizes) == 1:
            assert sizes[0] == op.workspace_bytes(C, 65, 2)
            op.reset_counts()
            assert op.counts() == (0, 0, 0)
            total[:] = 0
    assert sizes[0] < sizes[1] == sizes[2] and total[1] > 0
    op(accel.DeviceArray(ctx, (C, 0, 2), np.complex64), accel.DeviceArray(ctx, (C, 0, 2), np.float32),
       np.zeros(0, np.int32))
    assert op.counts() == tuple(total) and op.flags.shape == (C, 0, 2) and op.level.shape == (0, 2)
    # what the operator does not take
    vis = accel.DeviceArray(ctx, (C, 4, 2), np.complex64)
    weights = accel.DeviceArray(ctx, (C, 4, 2), np.float32)
    with pytest.raises(ValueError):
        op(vis, weights, np.zeros(3, np.int32))
    with pytest.raises(ValueError):
        op(vis, weights, np.zeros(4, np.float32))
    with pytest.raises(ValueError):
        op(accel.DeviceArray(ctx, (C + 1, 4, 2), np.complex64),
           accel.DeviceArray(ctx, (C + 1, 4, 2), np.float32), np.zeros(4, np.int32))
    with pytest.raises(TypeError):
        op(weights, weights, np.zeros(4, np.int32))
    assert op.counts() == tuple(total)


# ---- through the loader into the store --------------------------------------------------------------
def _read(coll, channel, w_slice):
    pieces = [p.copy() for p in coll.reader().iter_slice(channel, w_slice, None)]
    return np.rec.array(np.hstack(pieces)) if pieces else np.rec.recarray(0, coll.store_dtype)


def _assert_same_store(a, b, channels):
    assert a.num_input == b.num_input and a.num_output == b.num_output
    records = 0
    for channel in range(channels):
        assert a.reader().num_w_slices(channel) == b.reader().num_w_slices(channel)
        for s in range(a.reader().num_w_slices(channel)):
            x, y = _read(a, channel, s), _read(b, channel, s)
            assert len(x) == len(y)
            records += len(x)
            for field in ('uv', 'sub_uv', 'w_plane', 'weights', 'vis'):
                assert np.asarray(x[field]).tobytes() == np.asarray(y[field]).tobytes(), (channel, s, field)
    assert records > 20


def _make_band(C):
    """Two blocks of C channels: 4 baselines x 6 times in time order, two polarizations, noise of a
    different sigma on every baseline about a continuum, weights U(0.5, 1.5) with some zeros,
    spikes in both blocks and one baseline whose first block has no weight at all."""
    from katsdpimager_amd import loader
    ctx, q = context_queue()
    c = gi.E2E_CONFIGS['degrid']
    ip, gp, ap = make_params(c)
    baselines, times, P = 4, 6, 2
    R = baselines * times
    rng = np.random.default_rng(45)
    uvw = gi.e2e_raw(c)[0][:R]
    baseline = np.tile(np.arange(baselines), times)
    sigma = np.array([0.5, 1.0, 2.0, 4.0])[baseline]
    vis = ((rng.normal(size=(R, C, P)) + 1j * rng.normal(size=(R, C, P))) * sigma[:, None, None]
           + (2.0 - 1.0j)).astype(np.complex64)
    for r, ch, p in ((1, 2, 0), (6, 5, 1), (14, 1, 0), (21, 6, 1), (17, 3, 0)):
        vis[r, ch, p] += np.complex64(60.0 * sigma[r])
    weights = rng.uniform(0.5, 1.5, (R, C, P)).astype(np.float32)
    weights[rng.random((R, C, P)) < 0.1] = 0.0
    weights[:R // 2][baseline[:R // 2] == 3, :, 1] = 0.0
    freq = 1.4e9 + 1e6 * np.arange(C)
    dataset = loader.LoaderArrays(uvw, vis, weights, baseline, freq, [0, 1],
                                  longest_baseline=c['longest_baseline'])
    return dict(ctx=ctx, q=q, ip=ip, gp=gp, C=C, dataset=dataset, vis_load=C * R // 2,
                stokes=np.array([[0.5, 0.5]], np.complex64))


@pytest.fixture(scope='module')
def band():
    return _make_band(8)


@pytest.fixture(scope='module')
def long_band():
    """70 channels: three words of the operators' channel masks."""
    return _make_band(70)


def _collector(band, channels):
    from katsdpimager_amd import preprocess
    return preprocess.VisibilityCollectorDevice(band['q'], [band['ip']] * channels,
                                                [band['gp']] * channels, 1024)


def _through_and_by_hand(band, params, reweight, channels_out, operators, **keywords):
    """(the store of the loader with `keywords`, rfiflag=params and statwt=reweight; the store of the
    device operators of `keywords` run by hand, the twins of the flagger and of statwt chained after
    them and their output fed to the collector; the twins' total counts)."""
    from katsdpimager_amd import accel, loader, rfiflag, statwt
    ctx, q, C = band['ctx'], band['q'], band['C']
    through = _collector(band, channels_out)
    loader.preprocess_visibilities(band['dataset'], through, 0, C, (band['stokes'], None),
                                   vis_load=band['vis_load'], rfiflag=params, statwt=reweight, **keywords)
    by_hand = _collector(band, channels_out)
    ops = [make() for make in operators]
    flagged = np.zeros(3, np.int64)
    reweighted = np.zeros(2, np.int64)
    blocks = 0
    for chunk in loader.data_iter(band['dataset'], None, band['vis_load'], 0, C):
        vis = accel.DeviceArray(ctx, chunk['vis'].shape, np.complex64)
        weights = accel.DeviceArray(ctx, chunk['weights'].shape, np.float32)
        vis.set(q, chunk['vis'])
        weights.set(q, chunk['weights'])
        for op in ops:
            out = op(vis, weights)
            if out is not None:
                vis, weights = out
        host_vis = vis.get(q)
        new_weights, _, _, counts = rfiflag.rfiflag_host(host_vis, weights.get(q), chunk['baselines'], params)
        flagged += counts
        if reweight is not None:
            new_weights, _, counts = statwt.statwt_host(host_vis, new_weights, chunk['baselines'], reweight)
            reweighted += counts
        by_hand.add(chunk['uvw'], new_weights, host_vis, None, None, band['stokes'], None)
        blocks += 1
    by_hand.close()
    assert blocks == 2
    return through, by_hand, tuple(int(x) for x in flagged), tuple(int(x) for x in reweighted)


def test_between_the_continuum_fit_and_statwt_after_the_spectral_filter(band):
    from katsdpimager_amd import continuum, rfiflag, spectral, statwt
    C = band['C']
    smooth = spectral.SpectralParameters.average(2)
    cont = continuum.UVContSubParameters(0, line_ranges=[(1, 2)])
    params = rfiflag.RFIFlagParameters(3, max_window=2, line_ranges=[(1, 2)])
    reweight = statwt.StatWtParameters(3, line_ranges=[(1, 2)], min_samples=4)
    through, by_hand, flagged, reweighted = _through_and_by_hand(
        band, params, reweight, 4,
        [lambda: spectral.SpectralFilterTemplate(band['ctx'], smooth).instantiate(band['q'], C),
         lambda: continuum.UVContSubTemplate(band['ctx'], cont).instantiate(band['q'], 4)],
        spectral=smooth, continuum=cont)
    _assert_same_store(through, by_hand, 4)
    assert through.rfiflag_counts == flagged and through.statwt_counts == reweighted
    # per block 4 baselines of 3 rows, one group each, two polarizations; one pair without weight
    assert flagged[1] > 0 and flagged[2] >= 1 and sum(reweighted) == 2 * 4 * 2
    assert not hasattr(by_hand, 'rfiflag_counts')


def test_between_the_continuum_fit_and_statwt_with_line_ranges_on_the_mask_seams(long_band):
    """70 channels with the line ranges (30, 34) and (62, 66), across the seams at 32 and 64 of the
    three operators' masks alike: the store byte for byte the twins' chained by hand, and the three
    sets of counts."""
    from katsdpimager_amd import continuum, rfiflag, statwt
    band = long_band
    C = band['C']
    ranges = [(30, 34), (62, 66)]
    cont = continuum.UVContSubParameters(1, line_ranges=ranges)
    params = rfiflag.RFIFlagParameters(3, max_window=32, line_ranges=ranges)
    reweight = statwt.StatWtParameters(3, line_ranges=ranges, min_samples=4)
    through, by_hand, flagged, reweighted = _through_and_by_hand(
        band, params, reweight, C,
        [lambda: continuum.UVContSubTemplate(band['ctx'], cont).instantiate(band['q'], C)], continuum=cont)
    _assert_same_store(through, by_hand, C)
    assert through.rfiflag_counts == flagged and through.statwt_counts == reweighted
    from katsdpimager_amd import loader
    fitted = np.zeros(2, np.int64)
    for chunk in loader.data_iter(band['dataset'], None, band['vis_load'], 0, C):
        fitted += continuum.uvcontsub_host(chunk['vis'], chunk['weights'], cont)[2]
    # (the baseline without weight in the first block: three rows of one polarization)
    assert through.continuum_counts == tuple(fitted) == (2 * 12 * 2 - 3, 3)
    assert flagged[0] > 0 and flagged[1] > 0 and flagged[2] >= 1 and sum(reweighted) == 2 * 4 * 2
    assert not hasattr(by_hand, 'rfiflag_counts')


def test_alone(band):
    from katsdpimager_amd import rfiflag
    C = band['C']
    params = rfiflag.RFIFlagParameters(2, max_window=4)
    through, by_hand, flagged, _ = _through_and_by_hand(band, params, None, C, [])
    _assert_same_store(through, by_hand, C)
    assert through.rfiflag_counts == flagged and flagged[1] > 0 and flagged[2] >= 1
    assert not hasattr(through, 'statwt_counts')


# ---- through the driver ------------------------------------------------------------------------------
def test_driver_image_is_quieter_with_the_flagger():
    """A channel with injected bursts imaged without and with ``rfiflag=`` at its defaults: 60
    baselines of 30 integrations x 8 channels, a 1 Jy source, noise of sigma 1 under weights of 1;
    on every fourth baseline 5 integrations of channel 3 carry 30 more, on every fourth other one
    integration carries 10 more in every channel.  The rms of the dirty image of channel 3 away from
    the source must come out lower with the flagger; no factor is fixed.  (Measured on an MI355X:
    0.163843 without the flagger, 0.0369232 with it; 217 of 14400 samples flagged.)"""
    from katsdpimager_amd import frontend, imaging, loader, parameters, preprocess, rfiflag, weight
    ctx, q = context_queue()
    c = gi.E2E_CONFIGS['degrid']
    ip, gp, ap = make_params(c)
    C, R, channel = 8, 1800, 3
    rng = np.random.default_rng(9)
    uvw = gi.e2e_raw(c)[0][:R]
    baseline = np.arange(R) // 30                       # (e2e_raw: tracks of 30 consecutive rows)
    source = (20, -12)
    l, m = source[0] * c['pixel_size'], source[1] * c['pixel_size']
    n = np.sqrt(1 - l * l - m * m)
    uvw_wl = uvw.astype(np.float64) / c['wavelength']
    sky = 1.0 / n * np.exp(-2j * np.pi * (uvw_wl[:, 0] * l + uvw_wl[:, 1] * m + uvw_wl[:, 2] * (n - 1)))
    vis = sky[:, None] + rng.normal(size=(R, C)) + 1j * rng.normal(size=(R, C))
    for b in range(0, 60, 2):
        first = 30 * b + int(rng.integers(25))
        if b % 4 == 0:
            vis[first:first + 5, channel] += 30.0
        else:
            vis[first, :] += 10.0
    vis = vis.astype(np.complex64)[:, :, None]
    dataset = loader.LoaderArrays(uvw, vis, np.ones((R, C, 1), np.float32), baseline,
                                  1.4e9 + 1e6 * np.arange(C), [0], longest_baseline=c['longest_baseline'])
    wp = parameters.WeightParameters(weight.WeightType(c['weight_type']), c['robustness'])
    # (one minor cycle: the residual is the dirty image but for a tenth of one component)
    cp = parameters.CleanParameters(1, 0.1, c['major_gain'], c['threshold'], c['mode'], c['psf_cutoff'],
                                    c['psf_limit'], c['border'])
    im = imaging.ImagingTemplate(ctx, ap, ip.fixed, wp, gp.fixed, cp).instantiate(
        q, ip, gp, c['vis_block'], 0, 1)
    im.ensure_all_bound()
    G = c['pixels']
    away = np.ones((G, G), bool)
    y, x = G // 2 + source[1], G // 2 + source[0]
    away[y - 10:y + 11, x - 10:x + 11] = False
    away[:G // 8] = away[-(G // 8):] = False
    away[:, :G // 8] = away[:, -(G // 8):] = False
    rms = {}
    for label, keyword in (('without', None), ('with', rfiflag.RFIFlagParameters())):
        coll = preprocess.VisibilityCollectorDevice(q, [ip] * C, [gp] * C, 1024)
        loader.preprocess_visibilities(dataset, coll, 0, C, (np.identity(1, np.complex64), None),
                                       rfiflag=keyword)
        stats = frontend.process_channel(coll.reader(), channel, im, ip, gp, cp, wp.weight_type,
                                         c['vis_block'], 1, c['degrid'])
        assert stats is not None
        dirty = im.get_buffer('dirty')[0]
        rms[label] = float(np.sqrt(np.mean(np.square(dirty[away], dtype=np.float64))))
        if keyword is not None:
            kept, flagged, skipped = coll.rfiflag_counts
            print('rfiflag: {} kept, {} flagged, {} skipped'.format(kept, flagged, skipped))
            assert skipped == 0 and 75 + 15 * C <= flagged < 0.1 * R * C
    print('dirty-image rms away from the source: {:.6g} without the flagger, {:.6g} with it'.format(
        rms['without'], rms['with']))
    assert rms['with'] < rms['without']
