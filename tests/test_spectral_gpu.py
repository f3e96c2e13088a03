"""Spectral smoothing and channel averaging on the device (csrc/spectral.hip through
spectral.SpectralFilter) against the numpy twin (spectral.filter_host, tested on its own in
test_spectral_host.py), then through the loader into the store, with the other operators, and
through the example.

Device against twin, per real component: |dev - t| <= 2^-24 |t| + 1e-12 S, t the twin's float64
value BEFORE its one rounding and S the largest |v| among the window's usable inputs.  The first term
is the rounding the contract allows; the second covers float64 sums in another order or contracted
into FMAs, about L 2^-53 S = 8e-15 S at L = 72 (no cancellation in S1: g, w >= 0) -- two orders
inside the bound, while any float32 step lands near 6e-8 S and fails.  Weights:
|dev - t| <= 2^-24 |t| (1 + 1e-9).  The kept / flagged set and the two counters are exactly the
twin's.

What runs is listed in spectral_cases.py: SHAPES on every plane with the second stream and the
repeated calls; FORM_SHAPES, which take each of the six kernel forms past one round and one chunk
(test_spectral_host.py checks, without a device, that the two lists reach every branch of the
kernels' loops); and ABI_CASES, the (length, offset, step) that only a direct call of
kimg_spectral_filter can make, against the contract written out a second time.  Measured on an
MI355X over FORM_SHAPES and ABI_CASES (3.0 million float32 words, lengths up to 72): the largest
err / bound is 0.9995 for values and 0.99999 for weights, all of it the final float32 rounding, which
alone may use the whole first term; no error went past 2^-24 |t|, so the 1e-12 S term was not
drawn on at all, and every word had the bits of the truth rounded once -- the float64 differences
(L 2^-53 S) are too small to move a word across a float32 rounding boundary in so few samples."""
import itertools

import numpy as np
import pytest

import golden_inputs as gi
from helpers import context_queue, make_params, SENTINELS
from spectral_cases import (ABI_CASES, ABI_CHANNELS, FORM_PLANES, FORM_SHAPES, HANNING, SHAPES,
                            contract_double, random_block)
from spectral_cases import window as _span

pytestmark = pytest.mark.gpu

#: (N, Q): one element, partial / whole / whole + 1 waves, every polarization count, partial workgroups
PLANES = [(1, 1), (63, 1), (64, 1), (65, 1), (257, 2), (257, 3), (1000, 4)]


def _window(g, offset, step, o, C_in):
    """(i, c) of the inputs of output o that lie inside the band."""
    return _span(len(g), offset, step, o, C_in)


def _parameters(C_in, taps, bin):
    """The shape's parameters, with a coverage threshold that some set of inputs meets EXACTLY: the
    default 0.5 where the coefficients allow it (the dyadic ones do), else the coverage of the first
    half of the window of the output that _threshold_subset looks at -- of the part of it inside the
    band, where the band cuts it -- searched among the neighbours of cov / sum(g) so that the product
    rounds to cov."""
    from katsdpimager_amd.spectral import SpectralParameters
    params = SpectralParameters(taps, bin)
    if _threshold_subset(params, C_in) is not None:
        return params
    g, offset, step = params.coefficients()
    inside = [i for i, c in _window(g, offset, step, params.output_channels(C_in) // 2, C_in)]
    cov = 0.0
    for i in inside[:len(inside) // 2 + 1]:
        cov += g[i]
    guess = cov / float(g.sum())
    for mc in [guess] + [np.nextafter(guess, d) for d in (0.0, 1.0)]:
        params = SpectralParameters(taps, bin, float(mc))
        if params.min_sum() == cov:
            assert _threshold_subset(params, C_in) is not None
            return params
    raise AssertionError('no coverage threshold that a set of taps meets exactly')


def _threshold_subset(params, C_in):
    """(o, usable i's): an output channel and a set of its in-band inputs whose coefficients, added
    in ascending order in float64, give exactly min_sum; None if there is none among the candidates
    (every subset of a short window, the prefixes of a long one)."""
    g, offset, step = params.coefficients()
    C_out = params.output_channels(C_in)
    o = C_out // 2
    inside = [i for i, c in _window(g, offset, step, o, C_in)]
    if len(inside) <= 9:
        candidates = [s for r in range(1, len(inside) + 1) for s in itertools.combinations(inside, r)]
    else:
        candidates = [tuple(inside[:r]) for r in range(1, len(inside) + 1)]
    for subset in candidates:
        cov = 0.0
        for i in subset:
            cov += g[i]
        if cov == params.min_sum():
            return o, subset
    return None


def _inputs(params, C, N, Q, seed):
    """test_uvcontsub_gpu._inputs: weights U(0.5, 2) with 20 % zeros, and, where the plane has room,
    hand-made samples: a negative weight, a NaN and an Inf at a positive weight, a sample one of
    whose windows has no usable input at all, and one whose window is exactly at the coverage
    threshold (and so kept)."""
    rng = np.random.default_rng(seed)
    vis, weights = random_block(rng, C, N, Q)
    v2, w2 = vis.reshape(C, N * Q), weights.reshape(C, N * Q)       # (views)
    g, offset, step = params.coefficients()
    marks = {}
    if N * Q >= 63:
        mid = C // 2
        w2[:, 3] = rng.uniform(0.5, 2.0, C)
        w2[mid, 3] = -1.5
        w2[:, 5] = rng.uniform(0.5, 2.0, C)
        v2[mid, 5] = complex(np.nan, 2.0)
        w2[:, 6] = rng.uniform(0.5, 2.0, C)
        v2[mid, 6] = complex(-1.0, np.inf)
        o, subset = _threshold_subset(params, C)
        # element 7: nothing usable in the window of output o, in three ways in turn
        for k, (i, c) in enumerate(_window(g, offset, step, o, C)):
            w2[c, 7] = 1.0
            if k % 3 == 0:
                w2[c, 7] = 0.0
            elif k % 3 == 1:
                w2[c, 7] = -0.75
            else:
                v2[c, 7] = complex(np.nan, np.nan)
        # element 9: exactly the subset usable
        for i, c in _window(g, offset, step, o, C):
            w2[c, 9] = rng.uniform(0.5, 2.0) if i in subset else 0.0
        marks = dict(unusable=(o, 7), threshold=(o, 9))
    return vis, weights, marks


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

    def assert_unchanged(self, q):
        """Inputs and padding come back bit for bit."""
        out = self.whole.get(q)
        assert np.array_equal(out.view(np.uint8), self.host.view(np.uint8)), 'the input block changed'


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _worst(err, bound, ratios, key):
    """Keeps in ratios[key] the largest err / bound seen (an error where the bound is 0 counts as inf)."""
    if ratios is not None and err.size:
        with np.errstate(divide='ignore', invalid='ignore'):
            r = np.where(err > 0, err / bound, 0.0)
        ratios[key] = max(ratios.get(key, 0.0), float(r.max()))


def _check_against_truth(got_vis, got_weights, vis, weights, truth, length, offset, step, ratios=None):
    """`truth`: (vis complex128, weights float64, kept) before the contract's one rounding."""
    want, want_weights, kept = truth
    assert got_vis.shape == want.shape and got_weights.shape == want.shape
    assert got_vis.dtype == np.complex64 and got_weights.dtype == np.float32
    # S: the largest |v| among the usable inputs of every output's window
    C_in, C_out = vis.shape[0], want.shape[0]
    usable = (weights > 0) & np.isfinite(vis.real) & np.isfinite(vis.imag)
    size = np.where(usable, np.abs(vis.astype(np.complex128)), 0.0)
    S = np.zeros(want.shape)
    for o in range(C_out):
        for i, c in _span(length, offset, step, o, C_in):
            S[o] = np.maximum(S[o], size[c])
    # the kept set: flagged samples are +0 in all three words, kept ones have a weight above 0
    assert np.array_equal(got_weights > 0, kept)
    assert not _bits(got_weights[~kept]).any() and not _bits(got_vis[~kept]).any()
    for part in ('real', 'imag'):
        t = getattr(want, part)[kept]
        d = getattr(got_vis, part)[kept].astype(np.float64)
        err = np.abs(d - t)
        bound = 2.0 ** -24 * np.abs(t) + 1e-12 * S[kept]
        _worst(err, bound, ratios, 'values')
        # (the rounding alone may use all of the first term; what an error takes of the second one)
        _worst(np.maximum(err - 2.0 ** -24 * np.abs(t), 0.0), 1e-12 * S[kept], ratios, 'second term')
        assert (err <= bound).all(), 'worst excess {:.3g}'.format(float((err - bound).max()))
    t = want_weights[kept]
    err = np.abs(got_weights[kept].astype(np.float64) - t)
    bound = 2.0 ** -24 * np.abs(t) * (1 + 1e-9)
    _worst(err, bound, ratios, 'weights')
    assert (err <= bound).all(), 'weights: worst excess {:.3g}'.format(float((err - bound).max()))
    n = int(kept.sum())
    if ratios is not None:
        # how many float32 words are not the truth's, rounded once: what the float64 sums in another
        # order or with another contraction move across a rounding boundary
        other = int((_bits(got_vis[kept]) != _bits(want[kept].astype(np.complex64))).sum()
                    + (_bits(got_weights[kept]) != _bits(want_weights[kept].astype(np.float32))).sum())
        ratios['words of other bits'] = ratios.get('words of other bits', 0) + other
        ratios['words'] = ratios.get('words', 0) + 3 * n
    return kept, (n, kept.size - n)


def _check_against_twin(got_vis, got_weights, vis, weights, params, ratios=None):
    from katsdpimager_amd import spectral
    g, offset, step = params.coefficients()
    return _check_against_truth(got_vis, got_weights, vis, weights,
                                spectral.filter_host_double(vis, weights, params), len(g), offset, step,
                                ratios)


def _on_padded_blocks(ctx, q, op, vis, weights):
    """op on padded channel pitches, different for the two arrays: the outputs on the host, after
    the checks of their shapes and of the inputs and their padding coming back bit for bit."""
    C_out, (C, N, Q) = op.num_channels_out, vis.shape
    d_vis = _PaddedBlock(ctx, q, vis, 5)
    d_weights = _PaddedBlock(ctx, q, weights, 11)
    out_vis, out_weights = op(d_vis.array, d_weights.array)
    assert out_vis.shape == (C_out, N, Q) and out_weights.shape == (C_out, N, Q)
    assert out_vis.tensor.is_contiguous() and out_weights.tensor.is_contiguous()
    got_vis, got_weights = out_vis.get(q), out_weights.get(q)
    d_vis.assert_unchanged(q)
    d_weights.assert_unchanged(q)
    return got_vis, got_weights


def _assert_marks(marks, kept, counts):
    """The hand-made samples of _inputs came out as they were made to."""
    if marks:
        C_out = kept.shape[0]
        o, j = marks['unusable']
        assert not kept.reshape(C_out, -1)[o, j]
        o, j = marks['threshold']
        assert kept.reshape(C_out, -1)[o, j]
        assert counts[0] >= 1 and counts[1] >= 1


@pytest.mark.parametrize('C,taps,bin', SHAPES)
def test_device_against_twin(C, taps, bin):
    from katsdpimager_amd import accel, spectral
    ctx, q = context_queue()
    side = ctx.create_command_queue()
    params = _parameters(C, taps, bin)
    template = spectral.SpectralFilterTemplate(ctx, params)
    C_out = params.output_channels(C)
    for i, (N, Q) in enumerate(PLANES):
        vis, weights, marks = _inputs(params, C, N, Q, 1000 * C + 10 * bin + i)
        op = template.instantiate(q, C)
        assert op.counts() == (0, 0) and op.num_channels_out == C_out
        got_vis, got_weights = _on_padded_blocks(ctx, q, op, vis, weights)
        kept, counts = _check_against_twin(got_vis, got_weights, vis, weights, params)
        assert sum(counts) == C_out * N * Q
        assert op.counts() == counts
        _assert_marks(marks, kept, counts)
        # dense inputs, a side stream, the same operator twice: the same bits, and the counts of an
        # operator add up over its calls; an empty block in between changes nothing
        op2 = template.instantiate(side, C)
        e_vis = accel.DeviceArray(ctx, vis.shape, np.complex64)
        e_weights = accel.DeviceArray(ctx, weights.shape, np.float32)
        e_vis.set(side, vis)
        e_weights.set(side, weights)
        for call in (1, 2):
            o_vis, o_weights = op2(e_vis, e_weights)
            assert np.array_equal(_bits(o_vis.get(side)), _bits(got_vis))
            assert np.array_equal(_bits(o_weights.get(side)), _bits(got_weights))
            assert op2.counts() == (call * counts[0], call * counts[1])
            empty = op2(accel.DeviceArray(ctx, (C, 0, Q), np.complex64),
                        accel.DeviceArray(ctx, (C, 0, Q), np.float32))
            assert empty[0].shape == (C_out, 0, Q) and empty[1].shape == (C_out, 0, Q)
        assert np.array_equal(_bits(e_vis.get(side)), _bits(vis))
        assert np.array_equal(_bits(e_weights.get(side)), _bits(weights))
        op2.reset_counts()
        assert op2.counts() == (0, 0)


@pytest.mark.parametrize('C,taps,bin', FORM_SHAPES)
def test_every_form_past_one_round_and_one_chunk(C, taps, bin):
    """The shapes that take every form of csrc/spectral.hip through all of its control flow (the
    list says what each is there for; test_spectral_host.py checks that the lists reach it all), under
    the bounds of the module docstring.  Prints the largest err / bound it met."""
    from katsdpimager_amd import spectral
    ctx, q = context_queue()
    params = _parameters(C, taps, bin)
    template = spectral.SpectralFilterTemplate(ctx, params)
    C_out = params.output_channels(C)
    ratios = {}
    for i, (N, Q) in enumerate(FORM_PLANES):
        vis, weights, marks = _inputs(params, C, N, Q, 1000 * C + 10 * bin + len(taps) + i)
        assert bool(marks) == (N * Q >= 63)
        op = template.instantiate(q, C)
        assert op.counts() == (0, 0) and op.num_channels_out == C_out
        got_vis, got_weights = _on_padded_blocks(ctx, q, op, vis, weights)
        try:
            kept, counts = _check_against_twin(got_vis, got_weights, vis, weights, params, ratios)
        finally:
            print('C_in {} length {} bin {} plane {}x{}: worst err / bound so far {}'.format(
                C, len(taps) + bin - 1, bin, N, Q, ratios))
        assert sum(counts) == C_out * N * Q
        assert op.counts() == counts
        _assert_marks(marks, kept, counts)


def test_the_entry_point_on_device_pointers():
    """An empty plane is a successful call that leaves outputs and counters alone; the refusals of the
    contract write nothing either."""
    import ctypes
    from katsdpimager_amd import accel
    from katsdpimager_amd._lib import lib
    ctx, q = context_queue()
    C, N = 8, 100
    vis = accel.DeviceArray(ctx, (C, N, 1), np.complex64)
    weights = accel.DeviceArray(ctx, (C, N, 1), np.float32)
    vis.zero(q)
    weights.zero(q)
    out_vis = accel.DeviceArray(ctx, (C, N, 1), np.complex64)
    out_weights = accel.DeviceArray(ctx, (C, N, 1), np.float32)
    host_v = np.full((C, N, 1), SENTINELS[np.dtype(np.complex64)], np.complex64)
    host_w = np.full((C, N, 1), SENTINELS[np.dtype(np.float32)], np.float32)
    out_vis.set(q, host_v)
    out_weights.set(q, host_w)
    counts = accel.DeviceArray(ctx, (2,), np.int64)
    counts.zero(q)
    g = np.array(HANNING, np.float64)

    def call(plane=N, C_out=C, vo=None, pitch=N, length=3, offset=1, step=1, min_sum=0.5):
        return lib().kimg_spectral_filter(
            vis.ptr, pitch, weights.ptr, N, C, out_vis.ptr if vo is None else vo, N, out_weights.ptr, N,
            C_out, plane, g.ctypes.data_as(ctypes.c_void_p), length, offset, step, min_sum, counts.ptr,
            q.handle)
    assert call(plane=0) == 0
    assert call(C_out=C + 1) == -10001
    assert call(pitch=N - 1) == -10001
    assert call(vo=vis.ptr + 8 * N) == -10001           # an output that starts inside an input
    assert call(offset=3) == -10001
    assert call(min_sum=0.0) == -10001
    assert call(step=65) == -10002
    assert counts.get(q).tolist() == [0, 0]
    assert np.array_equal(_bits(out_vis.get(q)), _bits(host_v))
    assert np.array_equal(_bits(out_weights.get(q)), _bits(host_w))
    # ... and the call itself: nothing usable anywhere (every weight is 0), everything flagged
    assert call() == 0
    assert counts.get(q).tolist() == [0, C * N]
    assert not _bits(out_vis.get(q)).any() and not _bits(out_weights.get(q)).any()


@pytest.mark.parametrize('length,offset,step', ABI_CASES)
def test_every_offset_on_device_pointers(length, offset, step):
    """kimg_spectral_filter takes any 0 <= offset < length and any length at step 1; the Python layer
    sends len(taps) // 2 and odd tap counts only.  Random coefficients that are not symmetric (a
    reversed or shifted tap order cannot pass), all four arrays padded, the truth the contract of the
    header written out in spectral_cases.contract_double (test_spectral_host.py holds it against the
    twin), the bounds those of the module docstring."""
    import ctypes
    from katsdpimager_amd import accel
    from katsdpimager_amd._lib import lib
    ctx, q = context_queue()
    C, N = ABI_CHANNELS, 65
    C_out = C // step
    rng = np.random.default_rng(10000 * step + 100 * length + offset)
    vis, weights = random_block(rng, C, N, 1)
    g = rng.uniform(0.1, 1.0, length)
    assert length < 3 or not np.array_equal(g, g[::-1])
    min_sum = 0.5 * float(g.sum())
    d_vis = _PaddedBlock(ctx, q, vis, 5)
    d_weights = _PaddedBlock(ctx, q, weights, 11)
    out_vis = _PaddedBlock(ctx, q, np.full((C_out, N, 1), SENTINELS[np.dtype(np.complex64)]), 3)
    out_weights = _PaddedBlock(ctx, q, np.full((C_out, N, 1), SENTINELS[np.dtype(np.float32)]), 7)
    counts = accel.DeviceArray(ctx, (2,), np.int64)
    counts.zero(q)
    assert lib().kimg_spectral_filter(
        d_vis.whole.ptr, N + 5, d_weights.whole.ptr, N + 11, C, out_vis.whole.ptr, N + 3,
        out_weights.whole.ptr, N + 7, C_out, N, g.ctypes.data_as(ctypes.c_void_p), length, offset, step,
        min_sum, counts.ptr, q.handle) == 0
    got = []
    for block in (out_vis, out_weights):
        whole = block.whole.get(q)
        assert np.array_equal(_bits(whole[:, N:]), _bits(block.host[:, N:])), 'output padding written'
        got.append(whole[:, :N].reshape(C_out, N, 1))
    d_vis.assert_unchanged(q)
    d_weights.assert_unchanged(q)
    truth = contract_double(vis, weights, g, offset, step, min_sum, C_out)
    ratios = {}
    try:
        kept, expected = _check_against_truth(got[0], got[1], vis, weights, truth, length, offset, step,
                                              ratios)
    finally:
        print('length {} offset {} step {}: worst err / bound {}'.format(length, offset, step, ratios))
    assert sum(expected) == C_out * N
    assert tuple(counts.get(q).tolist()) == expected


# ---- through the loader into the store --------------------------------------------------------------
T = (0.0021, -0.0013)       # the new phase centre of the second test, (ra, dec) in radians


def _band_arrays():
    """About 200 rows of 12 channels and two polarizations: random visibilities, weights
    U(0.5, 1.5) with some zeros.  (uvw [R][3], baseline [R], vis [R][C][2], weights [R][C][2])"""
    c = gi.E2E_CONFIGS['degrid']
    C, R, Q = 12, 200, 2
    rng = np.random.default_rng(33)
    uvw = gi.e2e_raw(c)[0][:R]
    baseline = np.arange(R) // 30                   # (e2e_raw: tracks of 30 consecutive rows)
    vis = (rng.normal(size=(R, C, Q)) + 1j * rng.normal(size=(R, C, Q))).astype(np.complex64)
    weights = rng.uniform(0.5, 1.5, (R, C, Q)).astype(np.float32)
    weights[rng.random((R, C, Q)) < 0.1] = 0.0
    weights[17, 1:7, 0] = 0.0                       # output samples without usable inputs
    return uvw, baseline, vis, weights


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
    assert records > 100


@pytest.fixture(scope='module')
def band():
    from katsdpimager_amd import loader, spectral
    ctx, q = context_queue()
    c = gi.E2E_CONFIGS['degrid']
    ip, gp, ap = make_params(c)
    uvw, baseline, vis, weights = _band_arrays()
    C = vis.shape[1]
    freq = 1.4e9 + 1e6 * np.arange(C)
    params = spectral.SpectralParameters.hanning(bin=2)
    dataset = loader.LoaderArrays(uvw, vis, weights, baseline, freq, [0, 1],
                                  longest_baseline=c['longest_baseline'])
    return dict(ctx=ctx, q=q, ip=ip, gp=gp, C=C, C_out=params.output_channels(C), params=params,
                dataset=dataset, stokes=np.array([[0.5, 0.5]], np.complex64), vis_load=C * 70)


def _collector(band):
    from katsdpimager_amd import preprocess
    return preprocess.VisibilityCollectorDevice(band['q'], [band['ip']] * band['C_out'],
                                                [band['gp']] * band['C_out'], 1024)


def test_through_the_loader_matches_the_operator_by_hand(band):
    from katsdpimager_amd import accel, loader, spectral
    ctx, q, C = band['ctx'], band['q'], band['C']
    through = _collector(band)
    assert loader.preprocess_visibilities(band['dataset'], through, 0, C, (band['stokes'], None),
                                          vis_load=band['vis_load'], spectral=band['params']) is through
    by_hand = _collector(band)
    op = spectral.SpectralFilterTemplate(ctx, band['params']).instantiate(q, C)
    blocks = 0
    for chunk in loader.data_iter(band['dataset'], None, band['vis_load'], 0, C):
        vis = accel.DeviceArray(ctx, chunk['vis'].shape, np.complex64)
        weights = accel.DeviceArray(ctx, chunk['weights'].shape, np.float32)
        vis.set(q, chunk['vis'])
        weights.set(q, chunk['weights'])
        out_vis, out_weights = op(vis, weights)
        by_hand.add(chunk['uvw'], out_weights.get(q), out_vis.get(q), None, None, band['stokes'], None)
        blocks += 1
    by_hand.close()
    assert blocks == 3
    _assert_same_store(through, by_hand, band['C_out'])
    assert through.spectral_counts == op.counts()
    assert sum(through.spectral_counts) == band['C_out'] * 200 * 2 and through.spectral_counts[1] >= 1
    assert not hasattr(through, 'continuum_counts') and not hasattr(through, 'phase_centre')
    assert not hasattr(by_hand, 'spectral_counts')
    from katsdpimager_amd import preprocess
    wrong = preprocess.VisibilityCollectorDevice(q, [band['ip']] * C, [band['gp']] * C, 1024)
    with pytest.raises(ValueError):                 # a collector made for the input channels
        loader.preprocess_visibilities(band['dataset'], wrong, 0, C, (band['stokes'], None),
                                       spectral=band['params'])


def test_with_phase_centre_and_continuum_in_the_documented_order(band):
    """Phase shift, spectral filter, continuum fit -- against the three operators applied by hand."""
    from katsdpimager_amd import accel, continuum, loader, phaseshift, spectral
    ctx, q, C, C_out = band['ctx'], band['q'], band['C'], band['C_out']
    dataset = band['dataset']
    cont = continuum.UVContSubParameters(1, line_ranges=[(2, 4)])
    through = _collector(band)
    loader.preprocess_visibilities(dataset, through, 0, C, (band['stokes'], None),
                                   vis_load=band['vis_load'], continuum=cont, phase_centre=T,
                                   spectral=band['params'])
    by_hand = _collector(band)
    inv_wavelength = phaseshift.inverse_wavelengths([dataset.frequency(ch) for ch in range(C)])
    shift = phaseshift.PhaseShiftTemplate(
        ctx, phaseshift.PhaseShiftParameters(dataset.phase_centre(), T)).instantiate(q, inv_wavelength)
    smooth = spectral.SpectralFilterTemplate(ctx, band['params']).instantiate(q, C)
    subtract = continuum.UVContSubTemplate(ctx, cont).instantiate(q, C_out)
    for chunk in loader.data_iter(dataset, None, band['vis_load'], 0, C):
        vis = accel.DeviceArray(ctx, chunk['vis'].shape, np.complex64)
        weights = accel.DeviceArray(ctx, chunk['weights'].shape, np.float32)
        uvw = accel.DeviceArray(ctx, chunk['uvw'].shape, np.float32)
        vis.set(q, chunk['vis'])
        weights.set(q, chunk['weights'])
        uvw.set(q, chunk['uvw'])
        new_uvw = shift(vis, uvw)
        out_vis, out_weights = smooth(vis, weights)
        subtract(out_vis, out_weights)
        by_hand.add(new_uvw.get(q), out_weights.get(q), out_vis.get(q), None, None, band['stokes'], None)
    by_hand.close()
    _assert_same_store(through, by_hand, C_out)
    assert through.spectral_counts == smooth.counts()
    assert through.continuum_counts == subtract.counts()
    assert through.phase_centre == T


# ---- the example ------------------------------------------------------------------------------------
def test_example_shows_the_line_at_a_quarter_a_half_and_a_quarter():
    """examples/image_channel.py --spectral hanning at a small size: the line put into input channel
    4 has 1/4, 1/2, 1/4 of its dirty peak in output channels 3, 4, 5, within the 1e-4 relative that
    the project's image parity uses (the visibilities are exact multiples; the weights, 1 / 0.375 of
    the input's, rescale the imaging weights by a factor that robust weighting divides out again up to
    float32 rounding), and the other channels hold zeros."""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        'examples', 'image_channel.py')
    spec = importlib.util.spec_from_file_location('image_channel_example_spectral', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    peaks = mod.main(['--pixels', '512', '--vis', '160000', '--minor', '10', '--vis-block', '65536',
                      '--spectral', 'hanning'])
    assert peaks['expected'].tolist() == [0, 0, 0, 0.25, 0.5, 0.25, 0, 0]
    assert peaks['input'] > 0.5
    for o, share in ((3, 0.25), (4, 0.5), (5, 0.25)):
        ratio = peaks[o] / peaks['input']
        print('output channel {}: {:.8f} of the input'.format(o, ratio))
        assert abs(ratio - share) <= 1e-4 * share
    for o in (0, 1, 2, 6, 7):
        assert peaks[o] == 0.0
