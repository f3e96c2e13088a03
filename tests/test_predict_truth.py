"""Direct (DFT) prediction, kimg_predict, against a float64 truth across its shape space.

The predictor's other tests (test_hip_parity.py) use one configuration: P = 3, 25 sources, 301
visibilities, compared norm-wise at 2e-3.  No source-chunk boundary (the kernel stages sources
through LDS 256 at a time), no other polarization count and no visibility count around the
256-thread block is compared with anything there.  This module does that.

Contract (include/kimg.h), restated here in numpy: u_f = fl(fl(u ov + sub_u + 0.5) uv_scale),
bit-exact in numpy float32 (the integer and the + 0.5 are exact); w_f = fl(fl(w_plane w_scale) +
w_bias); phi = fl(fl(fl(l u_f) + fl(m v_f)) + fl((n-1) w_f)) in turns; t = v_fract(phi);
c = v_cos(t), s = v_sin(t) (argument in turns); acc = fmaf(c, f, acc), fmaf(-s, f, acc) over the
sources in order; vis = fl(vis - fl(acc wgt)).

predict_truth64 takes u_f, v_f bit-exact from numpy float32, w = w_plane w_scale + w_bias and the
phase in float64 from the float32 inputs, reduces the phase to (-1/2, 1/2] exactly and returns
vis0 - wgt sum_s f_s exp(-2 pi i phi_s) in complex128.

predict_bound, per visibility and polarization, bounds |Re| and |Im| of kernel - truth.  With
eps = 2^-24 and delta the hardware's absolute v_sin / v_cos error on [0, 1):
  - w: two roundings, |w_f - w| <= dw = 2 eps (|w_plane w_scale| + |w_bias|).
  - phase: five roundings over a = |l u_f| + |m v_f| + |(n-1) w|, each at most eps of a partial
    sum no larger than a (up to the |n-1| dw carried in), so |phi_f - phi| <= dphi =
    (3 eps a + |n-1| dw)(1 + 4 eps) + eps; the last eps covers v_fract of a tiny negative phase,
    which lands within 2^-24 of 1 (v_fract itself is otherwise exact).
  - cos / sin: both are 2 pi-Lipschitz in turns, so each term f c differs from its truth by at
    most |f| (2 pi dphi + delta); summed over the sources, T.
  - accumulation: the fma of source k rounds once, by at most eps |S^_k| with S^_k the computed
    partial sum; |S^_k| <= |S_k| + T + R with S_k the partial sum of the truth's terms and R the
    total rounding, so R <= (eps sum_k |S_k| + S eps T) / (1 - S eps), with sum_k |S_k| taken as
    the larger of the real and imaginary parts' sums.  (The cruder S eps sum|f| of the same
    derivation is ~50 times looser at S ~ 1000: it would sit within a factor of 5 of one
    source's contribution.)  Padding sources of the LDS chunks add exact zeros.  A = T + R.
  - last step: two roundings, so the bound is |wgt| A + 3 eps (|vis0| + |wgt| (|acc| + A)), the
    3 eps covering 2 eps (1 + eps).
Inputs of the bounded cases keep this well below one source's contribution: |flux| in [0.5, 1.5],
at most ~1000 sources, phases of at most ~35 turns (a T of ~0.03 at S = 1027).

The oracle (oracle.kimg_oracle.predict, the reference's _predict_host restated in C) forms the
same float32 phase, then cos / sin of fl(fl(-2 pi) phi) in double, rounded to float, and
accumulates unfused: it lies within predict_bound + |wgt| sum_s |f_s| (4 pi eps a_s + 3 eps) of
the truth (oracle_extra).

delta is measured (test_sin_cos_error_is_delta): single sources with m = n - 1 = 0 and l a power
of two, so that phi_f = l u_f exactly, swept densely over +-6 and +-200 turns (2^18 points each).
Observed on an MI355X: max |v_cos - cos|, |v_sin - sin| = 2.59e-7 = 2^-21.9 (DELTA_OBSERVED);
DELTA, the delta of predict_bound, is twice that rounded up to a power of two, 2^-20.  The test
asserts the ceiling 2^-16 and DELTA.

The exact cases set lmn = 0: the phase is then exactly 0, and with v_cos(0) = 1, v_sin(0) = 0
(asserted here, not assumed), integer fluxes, weights and visibilities keep every partial sum
below 2^24, so the kernel must equal vis0 - wgt sum f bit for bit whatever the chunking.

CPU tests (no marker): the truth moves by more than 4x its bound under each simulated bug in
MUTATIONS on every bounded and exact GPU case's inputs, the premise of the exact cases holds, the
oracle host lies within its own bound, kimg_predict's argument checks, and PredictTemplate's
refusal of float64.  GPU tests are marked one by one."""
import ctypes
import functools
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from helpers import context_queue, relerr        # noqa: E402

EPS = 2.0 ** -24
DELTA_OBSERVED = 2.594e-7     # 2^-21.88, on an MI355X (test_sin_cos_error_is_delta)
DELTA = 2.0 ** -20            # the delta of predict_bound: 2 x DELTA_OBSERVED, rounded up
DELTA_CEILING = 2.0 ** -16
EXACT = float(1 << 24)
CHUNK = 256                 # sources per LDS stage of predict_kernel (grid.hip)
KIMG_EINVAL = -10001
KIMG_EUNSUPPORTED = -10002
PAIRS = 1 << 20             # (visibility, source) pairs per numpy block
PAD = 300                   # sentinel visibilities behind num_vis (more than one block)
SENTINEL_VIS = np.complex64(1.5e30 - 2.5e29j)


# ---------------------------------------------------------------------------------------------
# the contract in numpy

def coords(uv, w_plane, oversample, uv_scale, w_scale, w_bias, half=True):
    """u_f, v_f (float32, bit-exact as the kernel forms them) and w (float64 from the float32
    w_scale, w_bias)."""
    k = uv[:, :2].astype(np.int64) * oversample + uv[:, 2:].astype(np.int64)
    assert np.abs(k).max(initial=0) < 1 << 23
    kf = k.astype(np.float32)
    if half:
        kf = kf + np.float32(0.5)
    uvf = kf * np.float32(uv_scale)
    w = w_plane.astype(np.float64) * float(np.float32(w_scale)) + float(np.float32(w_bias))
    return uvf[:, 0].astype(np.float64), uvf[:, 1].astype(np.float64), w


def _blocks(n, S):
    step = max(1, PAIRS // max(S, 1))
    for a in range(0, n, step):
        yield slice(a, min(n, a + step))


def _turns(phi):
    """phi reduced exactly to (-1/2, 1/2]: cos / sin of 2 pi times it keep float64 accuracy."""
    return phi - np.rint(phi)


MUTATIONS = ('drop_first', 'drop_last', 'drop_256', 'drop_chunk_last', 'double_one',
             'flux_next_pol', 'weight_next_pol', 'sine_sign', 'no_w_term', 'no_half_cell',
             'skip_last_vis')
PHASE_MUTATIONS = ('sine_sign', 'no_w_term', 'no_half_cell')     # no bug at zero phase


def applies(mutation, P, S, zero_phase=False):
    if mutation in ('flux_next_pol', 'weight_next_pol') and P == 1:
        return False
    if mutation == 'drop_256' and S <= 256:
        return False
    return not (zero_phase and mutation in PHASE_MUTATIONS)


def _mutate(mutation, weights, flux):
    """Simulated bugs that change what is summed: (weights, flux) as the buggy kernel uses them."""
    S = len(flux)
    weights = np.asarray(weights, np.float64)
    flux = np.array(flux, np.float64)
    if mutation == 'drop_first':
        flux[0] = 0
    elif mutation == 'drop_last':
        flux[S - 1] = 0
    elif mutation == 'drop_256':
        flux[256] = 0
    elif mutation == 'drop_chunk_last':
        flux[np.minimum(np.arange(0, S, CHUNK) + CHUNK - 1, S - 1)] = 0
    elif mutation == 'double_one':
        flux[S // 2] *= 2
    elif mutation == 'flux_next_pol':
        flux = np.roll(flux, -1, axis=1)
    elif mutation == 'weight_next_pol':
        weights = np.roll(weights, -1, axis=1)
    return weights, flux


def predict_truth64(vis0, uv, w_plane, weights, lmn, flux, oversample, uv_scale, w_scale, w_bias,
                    mutation=None):
    """vis0 - wgt sum_s flux_s exp(-2 pi i (l u_f + m v_f + (n-1) w)), complex128 [N][P];
    `mutation` simulates one bug of MUTATIONS."""
    u, v, w = coords(uv, w_plane, oversample, uv_scale, w_scale, w_bias,
                     half=mutation != 'no_half_cell')
    weights, flux = _mutate(mutation, weights, flux)
    lmn = np.asarray(lmn, np.float64)
    sign = 1.0 if mutation == 'sine_sign' else -1.0
    wterm = mutation != 'no_w_term'
    n, P = vis0.shape
    acc = np.zeros((n, P), np.complex128)
    for b in _blocks(n, len(lmn)):
        phi = u[b, None] * lmn[:, 0] + v[b, None] * lmn[:, 1]
        if wterm:
            phi = phi + w[b, None] * lmn[:, 2]
        t = 2 * np.pi * _turns(phi)
        acc[b] = (np.cos(t) + 1j * sign * np.sin(t)) @ flux
    out = np.asarray(vis0, np.complex128) - weights * acc
    if mutation == 'skip_last_vis':
        out[-1] = vis0[-1]
    return out


def _terms(vis0, uv, w_plane, weights, lmn, flux, oversample, uv_scale, w_scale, w_bias, delta):
    """Per visibility and polarization: T (term errors), sum_k |S_k|, |acc|; and a (per pair)
    reduced to sum_s |f_s| a_s for oracle_extra."""
    u, v, w = coords(uv, w_plane, oversample, uv_scale, w_scale, w_bias)
    dw = 2 * EPS * (np.abs(w_plane.astype(np.float64) * float(np.float32(w_scale)))
                    + abs(float(np.float32(w_bias))))
    lmn = np.asarray(lmn, np.float64)
    f = np.asarray(flux, np.float64)
    af = np.abs(f)
    n, P = vis0.shape
    T, partial, acc, fa = (np.zeros((n, P)) for _ in range(4))
    for b in _blocks(n, len(lmn)):
        a = (np.abs(u[b, None] * lmn[:, 0]) + np.abs(v[b, None] * lmn[:, 1])
             + np.abs(w[b, None] * lmn[:, 2]))
        dphi = (3 * EPS * a + np.abs(lmn[:, 2]) * dw[b, None]) * (1 + 4 * EPS) + EPS
        T[b] = (2 * np.pi * dphi + delta) @ af
        fa[b] = a @ af
        t = 2 * np.pi * _turns(u[b, None] * lmn[:, 0] + v[b, None] * lmn[:, 1]
                                + w[b, None] * lmn[:, 2])
        c, s = np.cos(t), np.sin(t)
        for p in range(P):
            re = np.cumsum(c * f[:, p], axis=1)
            im = np.cumsum(-s * f[:, p], axis=1)
            partial[b, p] = np.maximum(np.abs(re).sum(axis=1), np.abs(im).sum(axis=1))
            acc[b, p] = np.hypot(re[:, -1], im[:, -1])
    return T, partial, acc, fa


def predict_bound(vis0, uv, w_plane, weights, lmn, flux, oversample, uv_scale, w_scale, w_bias,
                  delta=None):
    """Bound on |Re| and |Im| of (kernel - predict_truth64), [N][P] (derivation: module
    docstring)."""
    delta = DELTA if delta is None else delta
    S = len(lmn)
    T, partial, acc, _ = _terms(vis0, uv, w_plane, weights, lmn, flux, oversample, uv_scale,
                                w_scale, w_bias, delta)
    R = (EPS * partial + S * EPS * T) / (1 - S * EPS)
    A = T + R
    wgt = np.abs(np.asarray(weights, np.float64))
    return wgt * A + 3 * EPS * (np.abs(vis0) + wgt * (acc + A))


def oracle_extra(d):
    """What the oracle host may err beyond predict_bound (module docstring)."""
    _, _, _, fa = _terms(d['vis0'], d['uv'], d['w_plane'], d['weights'], d['lmn'], d['flux'],
                         *_scales(d), 0.0)
    sf = np.abs(np.asarray(d['flux'], np.float64)).sum(axis=0)
    return np.abs(d['weights']) * (4 * np.pi * EPS * fa + 3 * EPS * sf)


def exact_truth(vis0, weights, flux, mutation=None):
    """At lmn = 0: vis0 - wgt sum_s flux_s (float64; exact for the integer inputs)."""
    weights, flux = _mutate(mutation, weights, flux)
    out = np.asarray(vis0, np.complex128) - weights * flux.sum(axis=0)
    if mutation == 'skip_last_vis':
        out[-1] = vis0[-1]
    return out


def _scales(d):
    return d['oversample'], d['uv_scale'], d['w_scale'], d['w_bias']


def _args(d):
    return (d['vis0'], d['uv'], d['w_plane'], d['weights'], d['lmn'], d['flux']) + _scales(d)


def deviation(got, want):
    """max(|Re|, |Im|) of the difference, per element."""
    dz = np.asarray(got, np.complex128) - want
    return np.maximum(np.abs(dz.real), np.abs(dz.imag))


# ---------------------------------------------------------------------------------------------
# cases

class Case:
    def __init__(self, name, P, S, n, seed=None):
        self.name, self.P, self.S, self.n = name, P, S, n
        self.seed = seed if seed is not None else zlib.crc32(name.encode()) & 0xffff

    def __repr__(self):
        return self.name


def _cnormal(rs, shape, scale):
    return (scale * (rs.standard_normal(shape) + 1j * rs.standard_normal(shape))).astype(np.complex64)


def _uv(rs, n, cells, oversample):
    """(u, v, sub_u, sub_v) int16, cells in [-cells, cells] (both signs), sub-cells in [0, ov)
    with both ends present."""
    uv = np.empty((n, 4), np.int16)
    uv[:, :2] = rs.randint(-cells, cells + 1, (n, 2))
    uv[:, 2:] = rs.randint(0, oversample, (n, 2))
    uv[0::5, 2] = 0
    uv[1::5, 2] = oversample - 1
    uv[2::5, 3] = 0
    uv[3::5, 3] = oversample - 1
    return uv


def _w_plane(rs, n, W):
    wp = rs.randint(0, W, n)
    wp[0::7] = 0
    wp[1::7] = W - 1
    return wp.astype(np.int16)


def bounded_inputs(case):
    """Random l, m in +-0.25 with n - 1 = sqrt(1 - l^2 - m^2) - 1, |flux| in [0.5, 1.5] with
    random signs, weights in [0.5, 1.5] per polarization, uv of both signs up to 57 wavelengths
    and w in [-70, 76] (never 0) over 16 planes: |phase| <= ~33 turns."""
    rs = np.random.RandomState(case.seed)
    P, S, n = case.P, case.S, case.n
    lm = rs.uniform(-0.25, 0.25, (S, 2)).astype(np.float32)
    lmn = np.empty((S, 3), np.float32)
    lmn[:, :2] = lm
    lmn[:, 2] = np.sqrt(1.0 - np.sum(lm.astype(np.float64) ** 2, axis=1)) - 1.0
    flux = (rs.uniform(0.5, 1.5, (S, P)) * rs.choice([-1, 1], (S, P))).astype(np.float32)
    W = 16
    w_scale = 9.7
    return dict(vis0=_cnormal(rs, (n, P), 2.0), uv=_uv(rs, n, 12, 8), w_plane=_w_plane(rs, n, W),
                weights=rs.uniform(0.5, 1.5, (n, P)).astype(np.float32), lmn=lmn, flux=flux,
                oversample=8, uv_scale=0.55, w_scale=w_scale, w_bias=(0.5 - 0.5 * W) * w_scale + 3.1)


def exact_inputs(P, S, n):
    """lmn = 0; flux (s % 7 + 1)(p + 1), negative where s % 4 == 3; weights in {1, 2, 3}, never
    equal in neighbouring polarizations; vis0 in {-20..20} + i{-20..20}; uv, w_plane and scales
    as anywhere else."""
    rs = np.random.RandomState(1000 * P + S)
    s = np.arange(S)[:, None]
    weights = 1 + (rs.randint(0, 3, (n, 1)) + rs.randint(1, 3, (n, 1)) * np.arange(P)) % 3
    flux = ((s % 7 + 1) * (np.arange(P)[None, :] + 1) * np.where(s % 4 == 3, -1, 1))
    return dict(vis0=(rs.randint(-20, 21, (n, P)) + 1j * rs.randint(-20, 21, (n, P))).astype(np.complex64),
                uv=_uv(rs, n, 2000, 8), w_plane=_w_plane(rs, n, 32),
                weights=weights.astype(np.float32), lmn=np.zeros((S, 3), np.float32), flux=flux.astype(np.float32),
                oversample=8, uv_scale=0.37, w_scale=2.1, w_bias=-33.3)


BOUNDED = [Case('p%d_s%d' % (P, S), P, S, 2309 + 7 * P) for P in (1, 2, 3, 4)
           for S in (1, 5, 256, 257, 1027)]
EXACT_S = (1, 2, 3, 4, 5, 255, 256, 257, 511, 512, 513, 1000, 4099)
EXACT_N = (1, 255, 256, 257, 4097)
LONG_N = 65537
LONG_CASE = (2, 5)          # (P, S) of the long launch


@functools.lru_cache(maxsize=None)
def _bounded(case):
    d = bounded_inputs(case)
    return d, predict_truth64(*_args(d)), predict_bound(*_args(d))


@functools.lru_cache(maxsize=None)
def _exact(P, S, n):
    d = exact_inputs(P, S, n)
    return d, exact_truth(d['vis0'], d['weights'], d['flux'])


# ---------------------------------------------------------------------------------------------
# CPU: the harness checks itself

def test_matrix_covers_the_issue():
    assert {c.P for c in BOUNDED} == {1, 2, 3, 4}
    assert {1, 5, 256, 257, 1027} <= {c.S for c in BOUNDED}
    # every chunk shape: one source, a padded group, exactly one chunk, one past it, chunks of
    # chunks with ragged tails
    assert {1, 2, 3, 4, 5, 255, 256, 257, 511, 512, 513, 1000, 4099} <= set(EXACT_S)
    assert {1, 255, 256, 257, 4097} <= set(EXACT_N) and LONG_N > 65536


def _min_ratios(cases):
    """Smallest (over cases) of the largest (over elements) deviation / bound of each mutation."""
    out = {}
    for case in cases:
        d, want, bound = _bounded(case)
        for m in MUTATIONS:
            if applies(m, case.P, case.S):
                r = float((deviation(predict_truth64(*_args(d), mutation=m), want) / bound).max())
                out[m] = min(out.get(m, np.inf), r)
    return out


@pytest.mark.parametrize('P', (1, 2, 3, 4))
def test_truth_sees_every_simulated_bug(P):
    """On the inputs of every bounded GPU case the truth moves some element by more than 4x its
    bound under each simulated bug; on those of every exact case (bound 0) by at least 1."""
    ratios = _min_ratios([c for c in BOUNDED if c.P == P])
    print('P=%d smallest deviation / bound:' % P, {m: round(r, 1) for m, r in ratios.items()})
    for m, r in ratios.items():
        assert r > 4, (m, r)
    assert set(ratios) == {m for m in MUTATIONS if applies(m, P, 1027)}
    for P_, S, n in _exact_cases():
        if P_ != P:
            continue
        d, want = _exact(P, S, n)
        for m in MUTATIONS:
            if applies(m, P, S, zero_phase=True):
                got = exact_truth(d['vis0'], d['weights'], d['flux'], mutation=m)
                assert deviation(got, want).max() >= 1, (S, n, m)


def _exact_cases():
    return [(P, S, n) for P in (1, 2, 3, 4) for S in EXACT_S for n in EXACT_N] + [LONG_CASE + (LONG_N,)]


def test_premise_exact_cases():
    """Every partial sum of every exact case stays below 2^24: |acc| <= sum |f|, the product with
    the weight and the result below |vis0| + wgt sum |f|, and all are integers."""
    for P, S, n in _exact_cases():
        d, want = _exact(P, S, n)
        top = (np.abs(d['vis0'].view(np.float32)).max()
               + d['weights'].max() * np.abs(d['flux']).sum(axis=0).max())
        assert top < EXACT, (P, S, n)
        assert np.all(d['flux'] == np.round(d['flux'])) and np.all(d['flux'] != 0)
        assert np.all(d['weights'] == np.round(d['weights']))
        assert np.all(want.real == np.round(want.real)) and np.all(want.imag == np.round(want.imag))


def test_truth_at_zero_phase_is_the_integer_sum():
    """predict_truth64 and exact_truth agree where both apply (lmn = 0)."""
    for P, S in ((1, 5), (3, 257), (4, 513)):
        d = exact_inputs(P, S, 300)
        assert np.array_equal(predict_truth64(*_args(d)),
                              exact_truth(d['vis0'], d['weights'], d['flux']))


def test_truth_agrees_with_a_direct_sum():
    """The blocked, phase-reduced truth against a plain complex exponential on a small case."""
    d = bounded_inputs(Case('direct', 3, 257, 200, seed=5))
    u, v, w = coords(d['uv'], d['w_plane'], *_scales(d))
    lmn = d['lmn'].astype(np.float64)
    phi = u[:, None] * lmn[:, 0] + v[:, None] * lmn[:, 1] + w[:, None] * lmn[:, 2]
    want = d['vis0'] - d['weights'] * (np.exp(-2j * np.pi * phi) @ d['flux'].astype(np.float64))
    assert np.abs(predict_truth64(*_args(d)) - want).max() < 1e-9


@pytest.mark.parametrize('case', BOUNDED, ids=repr)
def test_oracle_host_within_its_bound(case):
    """The oracle host (same float32 phase, double cos / sin, unfused accumulation) lies within
    predict_bound + oracle_extra of the truth."""
    d, want, bound = _bounded(case)
    host = _run_oracle(d)
    assert (deviation(host, want) / (bound + oracle_extra(d))).max() <= 1


def _run_oracle(d):
    from oracle import kimg_oracle as orc
    host = d['vis0'].copy()
    orc.predict(host, d['uv'][:, :2], d['uv'][:, 2:], d['w_plane'], d['weights'], d['lmn'],
                d['flux'], *_scales(d))
    return host


def test_predict_abi_argument_checks():
    """kimg_predict's argument checks, which return before any HIP call."""
    from katsdpimager_amd import build
    from katsdpimager_amd._lib import lib
    build.build_lib()
    L = lib()
    one = ctypes.c_void_p(1)

    def call(vis=one, uv=one, wp=one, wt=one, lmn=one, flux=one, n=4, S=3, P=1):
        return L.kimg_predict(vis, uv, wp, wt, lmn, flux, n, S, P, 8, 0.5, 1.0, 0.0, None)

    for P in (0, 5, -1):
        assert call(P=P) == KIMG_EUNSUPPORTED, P
    assert call(n=-1) == KIMG_EINVAL
    assert call(S=-1) == KIMG_EINVAL
    assert call(lmn=None) == KIMG_EINVAL
    assert call(flux=None) == KIMG_EINVAL
    for name in ('vis', 'uv', 'wp', 'wt'):
        assert call(**{name: None}) == KIMG_EINVAL, name
    # no-ops (predict.py:387-388): nothing is launched, lmn / flux may be NULL
    assert call(n=0) == 0
    assert call(S=0) == 0
    assert call(n=0, lmn=None, flux=None) == 0
    assert call(S=0, lmn=None, flux=None) == 0


def test_predict_template_rejects_float64():
    from katsdpimager_amd import predict
    with pytest.raises(ValueError, match='PredictTemplate'):
        predict.PredictTemplate(None, np.float64, 1)


# ---------------------------------------------------------------------------------------------
# GPU harness

def _dev(ctx, q, a):
    from katsdpimager_amd import accel
    a = np.ascontiguousarray(a)
    d = accel.DeviceArray(ctx, a.shape, a.dtype)
    d.set(q, a)
    return d


def run_predict(ctx, q, d, num_vis=None, num_sources=None, pad=PAD):
    """kimg_predict on d's first num_vis visibilities and num_sources sources, with `pad`
    sentinel visibilities behind them (vis SENTINEL_VIS, weights NaN); checks that the sentinels
    come back bit-identical and returns vis [num_vis][P]."""
    from katsdpimager_amd._lib import check, lib
    n = len(d['vis0']) if num_vis is None else num_vis
    S = len(d['lmn']) if num_sources is None else num_sources
    P = d['vis0'].shape[1]
    vis = np.concatenate([d['vis0'][:n], np.full((pad, P), SENTINEL_VIS)])
    weights = np.concatenate([d['weights'][:n], np.full((pad, P), np.nan, np.float32)])
    uv = np.concatenate([d['uv'][:n], np.zeros((pad, 4), np.int16)])
    wp = np.concatenate([d['w_plane'][:n], np.zeros(pad, np.int16)])
    bufs = [_dev(ctx, q, a) for a in (vis, uv, wp, weights, d['lmn'], d['flux'])]
    rc = lib().kimg_predict(*[b.ptr for b in bufs], n, S, P, *_scales(d), q.handle)
    check(rc, 'kimg_predict')
    q.finish()
    out = bufs[0].get(q)
    assert np.array_equal(out[n:].view(np.uint32), vis[n:].view(np.uint32)), 'beyond num_vis'
    return out[:n]


def _assert_exact(got, want, what):
    bad = got.astype(np.complex128) != want
    assert not bad.any(), '%s: %d values differ, first at %s: got %s, want %s' % (
        what, int(bad.sum()), np.argwhere(bad)[0], got[tuple(np.argwhere(bad)[0])],
        want[tuple(np.argwhere(bad)[0])])


@pytest.mark.gpu
@pytest.mark.parametrize('S', EXACT_S)
@pytest.mark.parametrize('P', (1, 2, 3, 4))
def test_predict_exact_at_zero_phase(P, S):
    """lmn = 0: vis0 - wgt sum f bit for bit at every visibility count around the block."""
    ctx, q = context_queue()
    for n in EXACT_N:
        d, want = _exact(P, S, n)
        _assert_exact(run_predict(ctx, q, d), want, 'P=%d S=%d n=%d' % (P, S, n))


@pytest.mark.gpu
def test_predict_exact_long_launch():
    ctx, q = context_queue()
    d, want = _exact(*LONG_CASE, LONG_N)
    _assert_exact(run_predict(ctx, q, d), want, 'long launch')


@pytest.mark.gpu
def test_predict_no_ops_leave_vis_untouched():
    """num_vis = 0 and num_sources = 0 change no bit of vis (lmn, flux valid or NULL)."""
    from katsdpimager_amd._lib import lib
    ctx, q = context_queue()
    d, _ = _exact(3, 257, 257)
    got = run_predict(ctx, q, d, num_vis=0)
    assert got.shape == (0, 3)
    got = run_predict(ctx, q, d, num_sources=0)
    assert np.array_equal(got.view(np.uint32), d['vis0'].view(np.uint32))
    vis = _dev(ctx, q, d['vis0'])
    bufs = [_dev(ctx, q, d[k]) for k in ('uv', 'w_plane', 'weights')]
    assert lib().kimg_predict(vis.ptr, *[b.ptr for b in bufs], None, None, 257, 0, 3,
                              *_scales(d), q.handle) == 0
    q.finish()
    assert np.array_equal(vis.get(q).view(np.uint32), d['vis0'].view(np.uint32))


def _delta_inputs(l, n=1 << 18):
    """One source at (l, 0, 0), l a power of two, unit flux and weight, vis0 = 0: the kernel then
    returns (-v_cos(t), v_sin(t)) with t = fract(l u_f) and u_f sweeping n values of both signs."""
    k = np.arange(n, dtype=np.int64) - n // 2
    ov = 4
    uv = np.zeros((n, 4), np.int16)
    uv[:, 0] = np.floor_divide(k, ov)
    uv[:, 2] = np.mod(k, ov)
    uv[:, 1] = -k[::-1] // 64
    return dict(vis0=np.zeros((n, 1), np.complex64), uv=uv, w_plane=(np.arange(n) % 8).astype(np.int16),
                weights=np.ones((n, 1), np.float32), lmn=np.array([[l, 0, 0]], np.float32),
                flux=np.ones((1, 1), np.float32), oversample=ov, uv_scale=0.7719 * 2.0 ** -14,
                w_scale=1.3, w_bias=-4.1)


@pytest.mark.gpu
def test_sin_cos_error_is_delta():
    """delta measured: |v_cos(t) - cos(2 pi t)|, |v_sin(t) - sin(2 pi t)| over t = fract(phi)
    for phi = l u_f exactly, densely over +-6 turns (l = 1) and +-200 turns (l = 32)."""
    ctx, q = context_queue()
    worst = 0.0
    for l in (1.0, 32.0):
        d = _delta_inputs(l)
        u, _, _ = coords(d['uv'], d['w_plane'], *_scales(d))
        phi = l * u
        assert np.array_equal(phi, (np.float32(l) * u.astype(np.float32)).astype(np.float64))
        got = run_predict(ctx, q, d)[:, 0]
        t = 2 * np.pi * _turns(phi)
        err = max(np.abs(-got.real - np.cos(t)).max(), np.abs(got.imag - np.sin(t)).max())
        print('l=%g: |phi| <= %.1f turns, max sin/cos error %.3e = 2^%.2f'
              % (l, np.abs(phi).max(), err, np.log2(err) if err else -np.inf))
        worst = max(worst, err)
    assert worst <= DELTA_CEILING
    assert worst <= DELTA


@pytest.mark.gpu
@pytest.mark.parametrize('case', BOUNDED, ids=repr)
def test_predict_within_bound(case):
    """General phase: every element within predict_bound of the truth, and within that bound plus
    the host's own of the oracle."""
    ctx, q = context_queue()
    d, want, bound = _bounded(case)
    got = run_predict(ctx, q, d)
    r = deviation(got, want) / bound
    print('%s: largest deviation / bound %.3f' % (case, r.max()))
    assert r.max() <= 1, np.unravel_index(np.argmax(r), r.shape)
    host = _run_oracle(d)
    assert (deviation(got, host) / (2 * bound + oracle_extra(d))).max() <= 1


def bench_inputs(n=20000, S=1000, P=1):
    """bench.py's predictor configuration: the synthetic observation's geometry (4096 pixels, 32
    W planes, oversample 8), S sources at +-0.4 of the image size, flux in [0.1, 1), w = 0."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import synth
    from katsdpimager_amd import predict
    obs = synth.make_observation(4096, n, 32, P, device='cpu', cover=0.30)
    ip, gp, _ = synth.make_parameters(obs, P, 28)
    uv_scale, w_scale, w_bias = predict.uvw_scale_bias(ip, gp)
    rs = np.random.RandomState(3)
    lm = rs.uniform(-0.4, 0.4, (S, 2)) * float(ip.image_size)
    lmn = np.concatenate([lm, np.sqrt(1 - np.sum(lm * lm, axis=1, keepdims=True)) - 1], axis=1)
    return dict(vis0=obs.vis.numpy().astype(np.complex64), uv=obs.uv.numpy(),
                w_plane=obs.w_plane.numpy(), weights=obs.weights.numpy().astype(np.float32),
                lmn=lmn.astype(np.float32), flux=rs.uniform(0.1, 1, (S, P)).astype(np.float32),
                oversample=gp.fixed.oversample, uv_scale=uv_scale, w_scale=w_scale, w_bias=w_bias)


@pytest.mark.gpu
def test_predict_bench_configuration():
    """S = 1000 at the bench's geometry (phases ~1e3 turns, where the bound is loose): HIP's
    element-wise and norm-wise error against the truth is at most 1.5x the oracle host's."""
    ctx, q = context_queue()
    d = bench_inputs()
    want = predict_truth64(*_args(d))
    got = run_predict(ctx, q, d)
    host = _run_oracle(d)
    assert np.abs(got - want).max() <= 1.5 * np.abs(host - want).max()
    err_hip = relerr(d['vis0'] - got, d['vis0'] - want)
    err_host = relerr(d['vis0'] - host, d['vis0'] - want)
    print('bench configuration vs float64: HIP %.3e, oracle host %.3e' % (err_hip, err_host))
    assert err_hip <= 1.5 * err_host
    assert (deviation(got, want) / predict_bound(*_args(d))).max() <= 1


def operator_inputs(n=3001, S=300, P=2):
    """1024 pixels of 2e-4 (l, m up to +-0.1), 16 W planes, w offset by set_w; 300 CLEAN
    components with |flux| in [0.5, 1.5] at distinct positions (two source chunks)."""
    import golden_inputs as gi
    c = gi.make_config(1024, 2e-4, 0.2, P, 7, 16, w_slices=4, max_w=50.0)
    rs = np.random.RandomState(17)
    cells = rs.choice(1024 * 1024, S, replace=False)
    comps = {(int(i) // 1024, int(i) % 1024):
             (rs.uniform(0.5, 1.5, P) * rs.choice([-1, 1], P)).astype(np.float32) for i in cells}
    return c, comps, dict(vis0=_cnormal(rs, (n, P), 2.0), uv=_uv(rs, n, 30, c['oversample']),
                          w_plane=_w_plane(rs, n, 16),
                          weights=rs.uniform(0.5, 1.5, (n, P)).astype(np.float32))


@pytest.mark.gpu
def test_predict_operator_set_sky_image():
    """Predict.set_sky_image with 300 components against the oracle's extract_sky_image and the
    truth; no components is a no-op; more than max_sources raises."""
    from helpers import make_params
    from katsdpimager_amd import predict
    from oracle import kimg_oracle as orc
    ctx, q = context_queue()
    c, comps, d = operator_inputs()
    ip, gp, _ = make_params(c)
    n, S, P = len(d['vis0']), len(comps), c['P']
    fn = predict.PredictTemplate(ctx, np.float32, P).instantiate(q, ip, gp, n + PAD, S)
    fn.ensure_all_bound()
    vis = np.concatenate([d['vis0'], np.full((PAD, P), SENTINEL_VIS)])
    fn.buffer('vis').set(q, vis)
    fn.buffer('uv').set_region(q, d['uv'], np.s_[:n], np.s_[:])
    fn.buffer('w_plane').set_region(q, d['w_plane'], np.s_[:n], np.s_[:])
    fn.buffer('weights').set_region(q, d['weights'], np.s_[:n], np.s_[:])
    fn.num_vis = n
    fn.set_sky_image(comps)
    assert fn.num_sources == S
    fn.set_w(7.25)
    fn()
    got = fn.buffer('vis').get(q)
    assert np.array_equal(got[n:].view(np.uint32), vis[n:].view(np.uint32))
    lmn, flux = orc.extract_sky_image(c['pixels'], c['pixel_size'], c['image_size'],
                                      c['oversample'], comps)
    assert np.array_equal(fn.buffer('lmn').get(q)[:S], lmn)
    assert np.array_equal(fn.buffer('flux').get(q)[:S], flux)
    uv_scale, w_scale, w_bias = predict.uvw_scale_bias(ip, gp)
    d.update(lmn=lmn, flux=flux, oversample=c['oversample'], uv_scale=uv_scale, w_scale=w_scale,
             w_bias=w_bias + 7.25)
    want, bound = predict_truth64(*_args(d)), predict_bound(*_args(d))
    assert (deviation(got[:n], want) / bound).max() <= 1
    # no components: nothing changes
    fn.buffer('vis').set(q, vis)
    fn.set_sky_image({})
    assert fn.num_sources == 0
    fn()
    assert np.array_equal(fn.buffer('vis').get(q).view(np.uint32), vis.view(np.uint32))
    more = dict(comps)
    more[(-1, -1)] = np.ones(P, np.float32)
    with pytest.raises(ValueError):
        fn.set_sky_image(more)
    with pytest.raises(ValueError):
        fn.set_sky_arrays(np.zeros((S + 1, 3)), np.zeros((S + 1, P)))
