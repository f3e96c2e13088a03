"""Statistical reweighting on the device (csrc/statwt.hip through statwt.StatWt) against the numpy
twin (statwt.statwt_host, tested on its own in test_statwt_host.py), then through the loader into the
store next to the other operators.

The contract fixes the order of every float64 sum and the build contracts nothing into fused
multiply-adds, so the device has the twin's bits: weights are compared as uint32 patterns, chi2 as
uint64 patterns (NaN in the same places), counts exactly.

The blocks come from statwt_cases.py: every band of SHAPES at 1, 63, 64, 65 and 1000 rows, 1 to 4
polarizations and time_bin 1, 3 and 64, baseline runs of 1 to 150 rows, 20 % zero weights, and
hand-made groups -- one exactly at min_samples (kept), one without any weight (flagged), a constant
one, and under the chi2 range one on either side of it -- which the twin is asserted to treat as
they were made to be treated.  A block of one row and one polarization is a single (group,
polarization) pair and holds the first of these only; a band of one fit channel in groups of one row
cannot reach two samples and holds no kept group at all."""
import numpy as np
import pytest

import band_cases as bands
import golden_inputs as gi
import statwt_cases as cases
from helpers import context_queue, make_params, SENTINELS

pytestmark = pytest.mark.gpu


class _PaddedBlock:
    """[C][N][P] inside a [C][pitch] device buffer of sentinels (test_uvcontsub_gpu._PaddedBlock)."""

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


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _assert_chi2(got, want):
    assert got.shape == want.shape and got.dtype == np.float64
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


def _run(ctx, q, op, vis, weights, ids):
    """op on padded channel pitches, different for the two arrays: (weights, chi2) on the host, the
    padding and the visibilities checked to be what they were."""
    d_vis = _PaddedBlock(ctx, q, vis, 5)
    d_weights = _PaddedBlock(ctx, q, weights, 11)
    op(d_vis.array, d_weights.array, ids)
    got = d_weights.get(q)
    assert np.array_equal(_bits(d_vis.get(q)), _bits(vis)), 'the visibilities changed'
    return got, op.chi2.get(q)


@pytest.mark.parametrize('shape', range(len(cases.SHAPES)))
def test_device_against_twin(shape):
    from katsdpimager_amd import statwt
    ctx, q = context_queue()
    C, mask = cases.SHAPES[shape]
    seen = set()
    for N in cases.ROWS:
        for P in cases.POLS:
            for time_bin in cases.TIME_BINS:
                vis, weights, ids, params, marks = cases.inputs(C, mask, N, P, time_bin,
                                                                1000 * shape + 10 * N + P)
                _, offsets, _, most = cases.parameters(C, mask, time_bin, ids)
                want, want_chi2, counts = statwt.statwt_host(vis, weights, ids, params)
                # the twin says of the hand-made groups what they were made for
                cases.assert_marks(marks, want, want_chi2, counts, weights, offsets, most, N, P)
                seen |= set(marks)
                op = statwt.StatWtTemplate(ctx, params).instantiate(q, C)
                assert op.counts() == (0, 0) and op.chi2 is None
                got, chi2 = _run(ctx, q, op, vis, weights, ids)
                where = (C, N, P, time_bin)
                assert np.array_equal(_bits(got), _bits(want)), where
                _assert_chi2(chi2, want_chi2)
                assert op.counts() == counts, where
    assert {'exact', 'empty', 'constant', 'samples'} <= seen


def _against_twin(ctx, q, C, mask, N, P, time_bin, seed):
    """One block of statwt_cases.inputs through the twin (whose answer for the hand-made groups is
    checked) and the device: bit equality; the marks it held."""
    from katsdpimager_amd import statwt
    vis, weights, ids, params, marks = cases.inputs(C, mask, N, P, time_bin, seed)
    _, offsets, _, most = cases.parameters(C, mask, time_bin, ids)
    want, want_chi2, counts = statwt.statwt_host(vis, weights, ids, params)
    cases.assert_marks(marks, want, want_chi2, counts, weights, offsets, most, N, P)
    op = statwt.StatWtTemplate(ctx, params).instantiate(q, C)
    got, chi2 = _run(ctx, q, op, vis, weights, ids)
    where = (C, N, P, time_bin)
    assert np.array_equal(_bits(got), _bits(want)), where
    _assert_chi2(chi2, want_chi2)
    assert op.counts() == counts, where
    return set(marks)


@pytest.mark.parametrize('C', bands.CHANNELS)
def test_device_against_twin_past_one_mask_word(C):
    """Every mask of band_cases with a fit channel, on both planes, time_bin 1, 3 and 64 in turn."""
    ctx, q = context_queue()
    seen, bins = set(), set()
    turn = 0
    for i, (name, mask) in enumerate(bands.masks(C)):
        for N, P in bands.PLANES:
            time_bin = cases.TIME_BINS[turn % 3]
            turn += 1
            try:
                seen |= _against_twin(ctx, q, C, mask, N, P, time_bin, 9000 * i + 10 * N + P + C)
            except AssertionError as e:
                raise AssertionError('{} at {}'.format(e, (C, name, N, P, time_bin))) from None
            bins.add(time_bin)
    assert turn >= 8 and bins == set(cases.TIME_BINS)
    assert {'exact', 'empty', 'constant'} <= seen


def test_one_launch_at_the_longest_band():
    """16384 channels, 512 words of mask by value in the kernel arguments of three launches: the only
    line channels are 8191, 8192 and two of the last word."""
    from katsdpimager_amd import continuum
    ctx, q = context_queue()
    C = continuum.MAX_CHANNELS
    assert C == 16384
    assert {'exact', 'empty', 'constant'} <= _against_twin(ctx, q, C, bands.limit_mask(C), 65, 2, 3, 16384)


def test_repeated_calls_and_a_growing_workspace():
    """The same operator on a small block, then, after reset_counts, on a larger one (the workspace
    grows) and on the small one again (it stays): each call has the twin's bits, the counts add up
    over calls and an empty block changes nothing."""
    from katsdpimager_amd import accel, statwt
    ctx, q = context_queue()
    C, mask = cases.SHAPES[0]
    small = cases.inputs(C, mask, 65, 2, 3, 77)
    large = cases.inputs(C, mask, 1000, 2, 3, 78)
    params = small[3]
    assert repr(large[3]) == repr(params)
    op = statwt.StatWtTemplate(ctx, params).instantiate(q, C)
    total = np.zeros(2, np.int64)
    sizes = []
    for vis, weights, ids, _, _ in (small, large, small):
        want, want_chi2, counts = statwt.statwt_host(vis, weights, ids, params)
        got, chi2 = _run(ctx, q, op, vis, weights, ids)
        assert np.array_equal(_bits(got), _bits(want))
        _assert_chi2(chi2, want_chi2)
        total += counts
        assert op.counts() == tuple(total)
        sizes.append(op._workspace.shape[0])
        if len(sizes) == 1:
            op.reset_counts()
            assert op.counts() == (0, 0)
            total[:] = 0
    assert sizes[0] < sizes[1] == sizes[2]
    op(accel.DeviceArray(ctx, (C, 0, 2), np.complex64), accel.DeviceArray(ctx, (C, 0, 2), np.float32),
       np.zeros(0, np.int32))
    assert op.counts() == tuple(total) and op.chi2.shape == (0, 2)
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


@pytest.fixture(scope='module')
def band():
    """Two blocks of 8 channels: 4 baselines x 6 times in time order, two polarizations, noise of a
    different sigma on every baseline, weights U(0.5, 1.5) with some zeros, and one baseline whose
    first block has no weight at all."""
    from katsdpimager_amd import loader
    ctx, q = context_queue()
    c = gi.E2E_CONFIGS['degrid']
    ip, gp, ap = make_params(c)
    C, baselines, times, P = 8, 4, 6, 2
    R = baselines * times
    rng = np.random.default_rng(44)
    uvw = gi.e2e_raw(c)[0][:R]
    baseline = np.tile(np.arange(baselines), times)
    sigma = np.array([0.5, 1.0, 2.0, 4.0])[baseline]
    vis = ((rng.normal(size=(R, C, P)) + 1j * rng.normal(size=(R, C, P))) * sigma[:, None, None]
           + (2.0 - 1.0j)).astype(np.complex64)
    weights = rng.uniform(0.5, 1.5, (R, C, P)).astype(np.float32)
    weights[rng.random((R, C, P)) < 0.1] = 0.0
    weights[:R // 2][baseline[:R // 2] == 3, :, 1] = 0.0
    freq = 1.4e9 + 1e6 * np.arange(C)
    dataset = loader.LoaderArrays(uvw, vis, weights, baseline, freq, [0, 1],
                                  longest_baseline=c['longest_baseline'])
    return dict(ctx=ctx, q=q, ip=ip, gp=gp, C=C, dataset=dataset, vis_load=C * R // 2,
                stokes=np.array([[0.5, 0.5]], np.complex64))


def _collector(band, channels):
    from katsdpimager_amd import preprocess
    return preprocess.VisibilityCollectorDevice(band['q'], [band['ip']] * channels,
                                                [band['gp']] * channels, 1024)


def _through_and_by_hand(band, params, channels_out, make_operator, **keywords):
    """(the store of the loader with `keywords` and statwt=params; the store of the same device
    operator of `keywords` run by hand, the twin's output blocks fed to the collector; the twin's
    total counts)."""
    from katsdpimager_amd import accel, loader, statwt
    ctx, q, C = band['ctx'], band['q'], band['C']
    through = _collector(band, channels_out)
    loader.preprocess_visibilities(band['dataset'], through, 0, C, (band['stokes'], None),
                                   vis_load=band['vis_load'], statwt=params, **keywords)
    by_hand = _collector(band, channels_out)
    op = make_operator()
    total = np.zeros(2, np.int64)
    blocks = 0
    for chunk in loader.data_iter(band['dataset'], None, band['vis_load'], 0, C):
        vis = accel.DeviceArray(ctx, chunk['vis'].shape, np.complex64)
        weights = accel.DeviceArray(ctx, chunk['weights'].shape, np.float32)
        vis.set(q, chunk['vis'])
        weights.set(q, chunk['weights'])
        out = op(vis, weights)
        if out is not None:
            vis, weights = out
        host_vis = vis.get(q)
        new_weights, _, counts = statwt.statwt_host(host_vis, weights.get(q), chunk['baselines'], params)
        total += counts
        by_hand.add(chunk['uvw'], new_weights, host_vis, None, None, band['stokes'], None)
        blocks += 1
    by_hand.close()
    assert blocks == 2
    return through, by_hand, tuple(int(x) for x in total)


def test_after_the_continuum_fit(band):
    from katsdpimager_amd import continuum, statwt
    C = band['C']
    cont = continuum.UVContSubParameters(0, line_ranges=[(3, 5)])
    params = statwt.StatWtParameters(2, line_ranges=[(3, 5)])
    through, by_hand, counts = _through_and_by_hand(
        band, params, C,
        lambda: continuum.UVContSubTemplate(band['ctx'], cont).instantiate(band['q'], C), continuum=cont)
    _assert_same_store(through, by_hand, C)
    # per block: 4 baselines of 3 rows in groups of 2 and 1, two polarizations; the baseline without
    # weight in the first block is flagged there, and so is every group of one row (6 samples)
    assert through.statwt_counts == counts and sum(counts) == 2 * 4 * 2 * 2
    assert counts[0] >= 8 and counts[1] >= 2
    assert not hasattr(by_hand, 'statwt_counts')


def test_after_the_spectral_filter(band):
    from katsdpimager_amd import spectral, statwt
    C = band['C']
    smooth = spectral.SpectralParameters.hanning(bin=2)
    params = statwt.StatWtParameters(3, fit_mask=[1, 0, 1, 1])
    through, by_hand, counts = _through_and_by_hand(
        band, params, 4,
        lambda: spectral.SpectralFilterTemplate(band['ctx'], smooth).instantiate(band['q'], C),
        spectral=smooth)
    _assert_same_store(through, by_hand, 4)
    assert through.statwt_counts == counts and sum(counts) == 2 * 4 * 2
    assert counts[0] >= 4 and counts[1] >= 1
