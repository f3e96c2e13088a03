"""Spectral smoothing and channel averaging without a device: the parameters object, the numpy twin
(spectral.filter_host, the executable form of the contract in include/kimg.h) against truths that do
not share its code, the noise it promises, the argument checks of kimg_spectral_filter (they run
before any HIP call), the ABI surface, and the loader's keyword; and, for test_spectral_gpu.py, that
the contract written out for the entry point's wider parameters (spectral_cases.contract_double) is
the twin's wherever both apply, and that the shapes it runs reach every form of csrc/spectral.hip and
every branch of its loops."""
import ctypes
import os
import re

import numpy as np
import pytest

import spectral_cases as cases
from spectral_cases import contract_double
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


# ---- the contract written out a second time, for the entry point's wider parameters ------------------
@pytest.mark.parametrize('C,taps,bin', cases.SHAPES + cases.FORM_SHAPES)
def test_contract_written_out_agrees_with_the_twin(C, taps, bin):
    """spectral_cases.contract_double (output by output, usable inputs only) against
    filter_host_double (tap by tap over all outputs, unusable inputs as zeros) wherever
    SpectralParameters reaches.  Both add the same float64 terms in ascending tap order, and an
    unusable input's +0.0 changes no bit of a sum, so the twin's own precision is: the same bits."""
    rng = np.random.default_rng(7 * C + bin)
    vis, weights = cases.random_block(rng, C, 5, 2)
    weights[C // 2, 1, 0] = -1.0
    vis[C // 3, 2, 1] = complex(np.nan, 1.0)
    vis[0, 3, 0] = complex(2.0, -np.inf)
    weights[:, 4, 1] = 0.0                              # windows with nothing usable at all
    params = SpectralParameters(taps, bin)
    g, offset, step = params.coefficients()
    want = filter_host_double(vis, weights, params)
    got = contract_double(vis, weights, g, offset, step, params.min_sum(), params.output_channels(C))
    assert not want[2][:, 4, 1].any() and want[2].any()
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert a.tobytes() == b.tobytes()


# ---- the shape lists of test_spectral_gpu.py against the dispatch of csrc/spectral.hip ---------------
def _kernel_constants():
    """SF_CHUNK, SF_UNROLL, {L: outputs per round} of the sliding instantiations, the longest filter
    and the largest bin, as csrc/spectral.hip and include/kimg.h state them."""
    from katsdpimager_amd import build
    source = open(os.path.join(build.CSRC, 'spectral.hip')).read()
    header = open(os.path.join(os.path.dirname(build.HERE), 'include', 'kimg.h')).read()
    const = {name: int(value)
             for name, value in re.findall(r'^constexpr int (SF_\w+) = (\d+);', source, re.M)}
    rounds = {int(L): int(L) * int(M) for L, M in re.findall(
        r'step == 1 && length == (\d+)\)\s*sliding\(integral_constant<int, \1>\{\}, '
        r'integral_constant<int, (\d+)>\{\}\);', source)}
    defines = dict(re.findall(r'^#define (KIMG_SPECTRAL_MAX_\w+) (\d+)$', header, re.M))
    largest_bin = int(defines['KIMG_SPECTRAL_MAX_BIN'])
    longest = int(defines['KIMG_SPECTRAL_MAX_TAPS']) + largest_bin - 1
    assert 'SF_MAX_LENGTH = KIMG_SPECTRAL_MAX_TAPS + KIMG_SPECTRAL_MAX_BIN - 1;' in source
    return const['SF_CHUNK'], const['SF_UNROLL'], rounds, longest, largest_bin


def _situations(C_in, length, offset, step, chunk, unroll, rounds, longest, largest_bin):
    """The dispatch at the end of kimg_spectral_filter and the loops of its kernels, restated: the
    form that (length, offset, step) selects, and what of that form's control flow C_in channels take
    it through.  A set of (form, situation)."""
    C_out = C_in // step
    assert C_out >= 1 and 0 <= offset < length <= longest
    if step == 1 and length in rounds:
        form = 'sliding {}'.format(length)
    elif offset == 0 and length == step:
        form = 'disjoint'
    else:
        form = 'window'
    found = set()
    spans = [(begin, min(C_out, begin + chunk)) for begin in range(0, C_out, chunk)]
    if len(spans) > 1:
        found.add('several chunks')
    for begin, end in spans:
        if begin > 0:
            found.add('a chunk that begins past output 0')
        if form.startswith('sliding'):
            R = rounds[length]
            # for (o0 = begin; o0 < end; o0 += R): prefetch if (o0 + R < end); outputs o0 + u < end
            prefetched = False
            for o0 in range(begin, end, R):
                partial = end - o0 < R
                if partial:
                    found.add('a partial last round')
                    if prefetched:
                        found.add('a partial round after a prefetch')
                if o0 + R < end:
                    found.add('a round with the prefetch taken')
                    prefetched = True
            if end - begin == R:
                found.add('a chunk of one exact round')
    if form != 'disjoint' and C_in < length:
        found.add('a band shorter than the window')
    if form != 'disjoint':
        found.add('offset {}'.format('first' if offset == 0 else 'last' if offset == length - 1
                                     else 'between'))
    if form == 'window':
        found.add('step 1' if step == 1 else 'step above 1')
    if not form.startswith('sliding'):
        # for (i0 = 0; i0 < length; i0 += unroll): taps i0 + u < length
        if length > unroll:
            found.add('several unroll groups, {}'.format('no remainder' if length % unroll == 0
                                                         else 'a remainder'))
        else:
            found.add('one unroll group')
        if C_in > C_out * step:
            found.add('input channels left over')
    if form == 'window' and length == longest:
        found.add('the longest filter')
    if form == 'disjoint' and length == largest_bin:
        found.add('the largest bin')
    return {(form, s) for s in found}


#: what the shape lists (C_in, taps, bin) have to reach ...
_LOOPS = ['several chunks', 'a chunk that begins past output 0']
_SLIDING = _LOOPS + ['a round with the prefetch taken', 'a partial last round',
                     'a partial round after a prefetch', 'a chunk of one exact round',
                     'a band shorter than the window']
_GROUPS = ['one unroll group', 'several unroll groups, no remainder', 'several unroll groups, a remainder',
           'input channels left over']
SHAPES_REACH = (
    [('sliding {}'.format(L), s) for L in (3, 5, 7, 9) for s in _SLIDING]
    + [('disjoint', s) for s in _LOOPS + _GROUPS + ['the largest bin']]
    + [('window', s) for s in _LOOPS + _GROUPS + ['a band shorter than the window', 'the longest filter']])
#: ... and the (length, offset, step) cases of the entry point
_OFFSETS = ['offset first', 'offset between', 'offset last']
ABI_REACH = (
    [('sliding {}'.format(L), s) for L in (3, 5, 7, 9) for s in _OFFSETS]
    + [('window', s) for s in _OFFSETS + ['step 1', 'step above 1']]
    + [('disjoint', 'one unroll group')])


def test_kernel_constants_are_the_ones_the_lists_were_written_for():
    chunk, unroll, rounds, longest, largest_bin = _kernel_constants()
    assert chunk == cases.CHUNK == 64 and unroll == 4 and longest == 72 and largest_bin == 64
    assert rounds == {3: 6, 5: 5, 7: 7, 9: 9}


def test_shape_lists_reach_every_form_and_every_branch_of_its_loops():
    """Shape lists rot: every (form, situation) of SHAPES_REACH must be met by some shape, and every
    shape of FORM_SHAPES must be the kind the dispatch takes it for (its place in the list)."""
    constants = _kernel_constants()
    reached = {}
    for C, taps, bin in cases.SHAPES + cases.FORM_SHAPES:
        g, offset, step = SpectralParameters(taps, bin).coefficients()
        for situation in _situations(C, len(g), offset, step, *constants):
            reached.setdefault(situation, []).append((C, len(g), step))
    missing = [s for s in SHAPES_REACH if s not in reached]
    assert not missing, 'no shape reaches {}'.format(missing)
    # the forms, in the order of the list's sections
    forms = []
    for C, taps, bin in cases.FORM_SHAPES:
        g, offset, step = SpectralParameters(taps, bin).coefficients()
        form = {f for f, s in _situations(C, len(g), offset, step, *constants)}.pop()
        if not forms or forms[-1] != form:
            forms.append(form)
    assert forms == ['sliding 3', 'sliding 5', 'sliding 7', 'sliding 9', 'disjoint', 'window']
    # a list that loses a shape which alone reaches a situation fails above: such shapes exist
    sole = {shapes[0] for shapes in reached.values() if len(shapes) == 1}
    assert (64 * 66 + 3, 72, 64) in sole and (4, 5, 1) in sole and (7, 7, 1) in sole


def test_entry_point_cases_reach_every_offset_of_every_form():
    constants = _kernel_constants()
    reached = set()
    for length, offset, step in cases.ABI_CASES:
        reached |= _situations(cases.ABI_CHANNELS, length, offset, step, *constants)
    missing = [s for s in ABI_REACH if s not in reached]
    assert not missing, 'no case reaches {}'.format(missing)
    assert len(set(cases.ABI_CASES)) == len(cases.ABI_CASES) == 24
    # lengths that SpectralParameters cannot make: even at step 1
    assert {(L, 1) for L in (2, 4, 6, 8)} <= {(length, step) for length, _, step in cases.ABI_CASES}


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
