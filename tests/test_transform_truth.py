"""The library's own mixed-radix transforms (csrc/image.hip: lds_fft, fft_stage_odd, fft_plan_for)
and the five entry points built on them, against a float64 truth at every layer size they accept.

    kimg_grid_to_image_real / kimg_image_to_grid_real   (w = 0, Hermitian fold, two rows per transform)
    kimg_grid_to_image_w    / kimg_image_to_grid_w      (any w)
    kimg_convolve_beam                                  (rows, columns forward x beam x inverse, rows)

Contract (include/kimg.h, next to the declarations), restated here: l = fl(fl(x lm_scale) +
lm_bias), n = sqrt(fl(1 - fl(fl(m m) + fl(l l)))), phase p = fl(w fl(n - 1)) turns reduced exactly
to r = p - rint(p), taper t = fl(k[y] k[x]); grid -> image writes fl(fl(v n) / t) with v the real
part of the (rotated) transform, image -> grid transforms fl(image / fl(t n)) (times c - i s); the
beam factor is fl(amplitude expf(power)) with power = fl(fl(fl(fl(a v) + fl(b u)) v) + fl(fl(c u) u)).

Truth.  transform_truth64 evaluates l, n, n - 1, p, r, t and `power` in float32 exactly as the
contract rounds them (numpy on the host, eager float32 torch on the device: the same IEEE
operations; test_device_float32_steps_match_numpy asserts they agree bit for bit) and everything
else -- every sum and product of the transforms, cos / sin / exp, the correction -- in float64.
Dense inputs take a complex128 FFT (numpy on the host, torch.fft on the device: another library,
another precision, none of this project's kernels); sparse inputs take the closed form, a sum of a
handful of outer products of exact-angle phase vectors.  The two are compared with each other and
with numpy (test_device_truth_agrees_with_numpy_and_closed_form).

Bound.  u = 2^-24.  A table twiddle or root constant is a double value rounded per component:
|w^ - w| <= mu = sqrt(2) u.  cmul's components are fma(a.x, b.x, -fl(a.y b.y)): one rounding of the
inner product and one of the fma, so |cmul(a, b) - a b| <= u (|a.y| |b| + |a b|) <= 2 u |a| |b|.
A complex addition errs by at most u times its result.  Per stage, the relative perturbation eta of
every term that enters an output (terms of modulus at most the l1 norm of the inputs under it):
  - radix 2: twiddle mu, cmul 2u, add u:                          eta_2  = mu + 3u
  - radix 4, first level (w1 = cmul(w2, w2): 2 mu + 2u; cmul 2u; add u):   eta_4a = 2 mu + 5u
    second level (cmul by w2: mu + 2u; times -+i exact; add u):          eta_4b = mu + 3u
  - radix r = 3, 5, 7: wk = w^k by repeated cmul, k <= r - 1: (r-1) mu + (r-2) 2u; cmul(wk, x) 2u;
    cmul(root, .) mu + 2u; r - 1 additions (r-1) u:                eta_r  = r mu + (3r - 1) u
Per element (sparse inputs): by induction over the stages every cell holds its exact partial sum
plus an error of at most (prod_s (1 + eta_s) - 1) times the l1 norm of the inputs under it, so
  |y^_c - y_c| <= E(G) ||x||_1,   1 + E(G) = (1 + 64u) prod_s (1 + eta_s)
(the 1 + 64u covers the second-order terms dropped from every eta).  E is 89 u at 4374 = 2 3^7.
Norm-wise (dense inputs; Higham, Accuracy and Stability, th. 24.2, with radix-r stages): a stage is
A_s + dA_s with |dA_s| <= eta_s |A_s|, ||A_s||_2 = sqrt(r), || |A_s| ||_2 = r, so
  ||y^ - y||_2 <= N(G) ||y||_2,   1 + N(G) = (1 + 64u) prod_s (1 + sqrt(r_s) eta_s)
(a radix-4 stage counts as its two radix-2 levels).  N is 154 u at 4374.
Two dimensions and the rest of each kernel (transform_bound):
  - the fold 0.5 (g + conj g') and the pairing of two rows (t.x - t.w ...) round once each: (1+u)^2;
    two real rows share a complex transform, so the l1 norm under a row's output is that of both
    rows: per-element bounds of the real pair and of the beam carry K = 2 (K = 4 for the beam,
    which packs twice); norm-wise the two rows are orthogonal and K = 1;
  - correction: fl(fl(v n) / t) with t = fl(k k) rounds three times: 3u; accumulate adds
    u (|old| + |out|);
  - any w: cos / sin of the exactly reduced float32 phase, taken to be within delta = 4u of the
    truth (the ceiling OpenCL sets for sincospi; the device library documents 1 - 2 ulp), two
    products and a subtraction: rot = sqrt(2) delta + 2u <= 8u, relative to |F|, the modulus
    of the complex transform -- so the any-w bounds are stated against |F|, not Re F;
  - image -> grid input: fl(image / fl(t n)) 3u (n is exact in the truth, which takes it in
    float32), times c, s: sqrt(2) delta + u <= 7u; the split 0.5 (z +- conj z') u;
  - beam: expf within 2 ulp, one product with amplitude, one with the cell: 6u of the largest
    factor Bmax; forward and inverse pairs of transforms: (1 + E)^4, against Bmax G^2 ||x||.
  grid -> image, per pixel:  K C ||g||_1 n / t,   1 + C = (1+u)^2 (1+E)^2 (1+3u) (1+rot)
  grid -> image, norm:       ||(y^ - y) t / n||_F <= C' ||F||_F,  C' with N for E
  image -> grid, per cell:   K C ||image / (t n)||_1;  norm: ||g^ - g||_F <= C' G ||image / (t n)||_F
  beam, per pixel: 4 C_b Bmax ||x||_1 (the 1 / G^2 being inside Bmax);  norm: C_b' Bmax G ... see code.
The constants are worst-case and therefore loose: rounding errors add like a random walk, not in
phase, so measured deviations sit near sqrt(stages) u where the bounds allow ~10 stages u sqrt(r).

Measured on one MI355X (largest deviation / bound per operation over all 241 sizes; size where it
occurred): MEASURED below, 0.033 at most; the FFT library's route ({'own_transform': False}) at
LIBRARY_SIZES: LIBRARY_ROUTE.  The float32 numpy model of lds_fft (same stage order,
digit reversal, float32 tables, root constants, cmul) stays within E and N at all 241 sizes, both
directions (test_model_within_bound); its largest ratios are in MODEL.

Simulated bugs (test_truth_sees_simulated_bugs, CPU): applied one at a time to the float32 model
(1-D bugs) or to a float64 restatement of the kernels' structure (fold, pairing, shifts, block
order, beam amplitude).  SEEN lists those whose deviation / bound exceeds 1 at every size where
they can act, with the smallest ratio; BELOW_BOUND lists those the worst-case bounds cannot see,
with their largest ratio -- that is what this module cannot notice.

Exact cases: a DC-only grid with kernel1d = 1, lm_scale = lm_bias = 0 (n = 1, which the entry
points accept) gives the constant image bit for bit (the cell's imaginary part vanishes in the fold
at w = 0 and meets s = 0 otherwise), accumulate 0 and 1; a single pixel at the image centre gives
a constant grid bit for bit: in both only the unit twiddle meets a non-zero cell.

GPU wall time on one MI355X: 68 s for the module (tests/test_hip_parity.py: 65 s on the same
machine).  The dense truths are matrix products with exact-angle phase matrices, so that no float64
FFT plan is made per size; torch.fft and numpy check them at a few sizes and at 8192.  Thinned
against the issue's matrix: one Gg per size and pair (the rule above); stride / accumulate / refusals /
beams at the seven REPRESENTATIVE sizes; w and bias cases with dense input at all of them and sparse
input for two of the six; the library route at LIBRARY_SIZES; structure bugs in a float64 restatement
at sizes up to 140.  The order test's second half (test_order_results_equal_one_size_at_a_time) needs
the first to have run in the same process."""
import functools
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

U = 2.0 ** -24
MU = math.sqrt(2.0) * U
DELTA = 4.0 * U
ROT = 8.0 * U
SECOND_ORDER = 1.0 + 64.0 * U
KIMG_EINVAL = -10001
OPS = ('g2i_real', 'i2g_real', 'g2i_w', 'i2g_w', 'beam')
REFUSED = ((14, 2), (17, 2), (22, 2), (8194, 2), (8748, 2), (64, 3), (64, 66), (64, 0))
REPRESENTATIVE = (16, 1024, 1458, 1250, 686, 5040, 8192)     # 2^k, 2 3^6, 2 5^4, 2 7^3, all, ends
W_ALL_SIZES = 117.25

# float32 model against E and N (test_model_within_bound): direction -> (per element, size, norm, size)
MODEL = {False: (0.031, 6720, 0.017, 64), True: (0.032, 576, 0.018, 16)}
# largest deviation / bound on one MI355X over all 241 sizes, as test_report_largest_ratios printed
# them: op -> ((per element, size), (norm-wise, size), (of the peak, size))
MEASURED = {
    'g2i_real': ((0.01124, 6272), (0.01201, 32), (4.988e-07, 5488)),
    'i2g_real': ((0.01441, 5292), (0.01171, 32), (5.654e-07, 2058)),
    'g2i_w': ((0.03275, 7000), (0.008336, 128), (5.559e-07, 7056)),
    'i2g_w': ((0.02902, 6860), (0.01189, 128), (6.161e-07, 2058)),
    'beam': ((0.0002456, 686), (0.006347, 1024), (9.604e-07, 8192)),
}
# the FFT library's route ({'own_transform': False}) at LIBRARY_SIZES, w = 0 grid -> image, the largest
# of its ratios: norm-wise 0.0106 at 8192, per element 0.0066 at 5040
LIBRARY_ROUTE = {'norm': (0.0106, 8192), 'element': (0.0066, 5040)}
# Simulated bugs, smallest .. largest ratio over all sizes where they act (test_truth_sees_simulated_bugs):
#   seen:    w1_is_w2, no_conj_2 > 1e3; perm_swapped 1.2e3 (4802) .. 1.05e5; last_cell 2.5e4 (168) ..
#            1.2e5; no_conj_3 8.5e4 .. 1.9e5; no_conj_5 8.6e4 .. 1.8e5; no_conj_7 1.0e5 .. 1.7e5
#   unseen:  twiddle_4ulp 0.011 .. 0.096 (196); table_float32 0.010 .. 0.042 (112);
#            root5_digits, root7_digits (6 decimals kept) 0.010 .. 0.031: the worst-case constants
#            are ~30 times what float32 does, so value bugs of a few ulps pass
#   no bug:  root5_literal, root7_literal (the float32 constant does not change); pair_nyquist
# Mutants of image.hip on the GPU (failed tests of this module's 287 / of the 36 cases of
# test_grid_to_image_real_transform_route, test_grid_image_own_transform_any_w and
# test_convolve_beam_own_transform): radix-7 root c[1] + 1e-4: 116 / 6; the last twiddle of the last
# radix-3 stage turned by 1e-4 rad: 165 / 12; the same root 2 ulps off: 0 / 0; `n == 0` for
# `n == 0 || 2 * n == G` in g2i_rows_kernel: 0 / 0 (no bug, see pair_nyquist)


# ---------------------------------------------------------------------------------------------
# sizes and plans, as fft_stages / fft_plan_for make them

def stages_of(G):
    """Radices of the stages for G cells (4s, at most one 2, 3s, 5s, 7s) or None."""
    twos, rest = 0, G
    while rest % 2 == 0:
        rest //= 2
        twos += 1
    radix = [4] * (twos // 2) + [2] * (twos % 2)
    for r in (3, 5, 7):
        while rest % r == 0:
            rest //= r
            radix.append(r)
    return radix if rest == 1 and radix and len(radix) <= 16 else None


def supported(G, Gg):
    return (16 <= G <= 8192 and G % 2 == 0 and stages_of(G) is not None
            and Gg >= 2 and Gg % 2 == 0 and Gg <= G)


SIZES = tuple(G for G in range(16, 8193, 2) if supported(G, 2))

ROOTS = {
    3: ((1.0, -0.5, -0.5), (0.0, 0.86602540378443865, -0.86602540378443865)),
    5: ((1.0, 0.30901699437494742, -0.80901699437494742, -0.80901699437494742, 0.30901699437494742),
        (0.0, 0.95105651629515357, 0.58778525229247313, -0.58778525229247313, -0.95105651629515357)),
    7: ((1.0, 0.62348980185873353, -0.22252093395631440, -0.90096886790241913, -0.90096886790241913,
         -0.22252093395631440, 0.62348980185873353),
        (0.0, 0.78183148246802981, 0.97492791218182361, 0.43388373911755812, -0.43388373911755812,
         -0.97492791218182361, -0.78183148246802981)),
}


@functools.lru_cache(maxsize=None)
def plan_for(G):
    """(radices, [(re, im) float32 twiddles of each stage], perm) exactly as fft_plan_for."""
    radix = stages_of(G)
    tw, radix2, q = [], [], 1
    for r in radix:
        angle = 2.0 * np.pi * np.arange(q, dtype=np.float64) / float(r * q)
        tw.append((np.cos(angle).astype(np.float32), np.sin(angle).astype(np.float32)))
        q *= r
        radix2 += [2, 2] if r == 4 else [r]
    n = np.arange(G)
    rem, block, pos = n.copy(), G, np.zeros(G, np.int64)
    for r in reversed(radix2):
        block //= r
        pos += (rem % r) * block
        rem //= r
    return tuple(radix), tw, pos


# ---------------------------------------------------------------------------------------------
# float32 model of lds_fft

def _cmul(ar, ai, br, bi):
    """cmul of image.hip: fma(a.x, b.x, -fl(a.y b.y)), fma(a.x, b.y, fl(a.y b.x)).  The fma is taken
    in float64 (the product of two float32 is exact there) and rounded to float32."""
    d = np.float64
    re = (ar.astype(d) * br.astype(d) - (ai * bi).astype(d)).astype(np.float32)
    im = (ar.astype(d) * bi.astype(d) + (ai * br).astype(d)).astype(np.float32)
    return re, im


def _ulps(value, k):
    v = np.float32(value)
    for _ in range(abs(k)):
        v = np.nextafter(v, np.float32(np.inf if k > 0 else -np.inf))
    return v


MODEL_BUGS = ('twiddle_4ulp', 'table_float32', 'root5_digits', 'root7_digits', 'root5_literal',
              'root7_literal', 'w1_is_w2', 'perm_swapped', 'last_cell', 'no_conj_3', 'no_conj_5',
              'no_conj_7', 'no_conj_2')


def bug_acts(bug, G, inverse):
    radix = stages_of(G)
    if bug.startswith('root') or bug.startswith('no_conj'):
        r = int(bug.split('_')[0][-1]) if bug.startswith('root') else int(bug[-1])
        if r == 2:
            return 4 in radix and not inverse        # (a lone radix-2 stage is the first: w = 1)
        return r in radix and (not bug.startswith('no_conj') or not inverse)
    if bug == 'w1_is_w2':
        return radix.count(4) >= 2          # (the first stage has w2 = 1)
    return True


def lds_fft_model(x, inverse, bug=None):
    """lds_fft<INVERSE> on the rows of x (B, G) complex: float32 throughout, the kernel's order."""
    x = np.atleast_2d(np.asarray(x, np.complex64))
    G = x.shape[1]
    radix, tw, perm = plan_for(G)
    perm = perm.copy()
    if bug == 'perm_swapped':
        perm[[G // 3, G // 3 + 1]] = perm[[G // 3 + 1, G // 3]]
    xr = np.zeros(x.shape, np.float32)
    xi = np.zeros(x.shape, np.float32)
    xr[:, perm] = x.real
    xi[:, perm] = x.imag
    roots = {r: (np.array(c, np.float32), np.array(s, np.float32)) for r, (c, s) in ROOTS.items()}
    for r, digits in ((5, 6), (7, 6)):
        if bug == 'root%d_digits' % r:      # the literal cut to 6 decimals
            roots[r][0][1] = np.float32(round(ROOTS[r][0][1], digits))
        if bug == 'root%d_literal' % r:     # the 17-digit literal with its last decimal dropped
            roots[r][0][1] = np.float32(float(repr(ROOTS[r][0][1])[:-1]))
    q = 1
    last = len(radix) - 1
    for stage, r in enumerate(radix):
        twr, twi = tw[stage][0].copy(), tw[stage][1].copy()
        if stage == last and bug == 'twiddle_4ulp':
            twr[q // 2 + (q > 1)] = _ulps(twr[q // 2 + (q > 1)], 4) if q > 1 else _ulps(twr[0], -4)
        if stage == last and bug == 'table_float32':
            a32 = (np.float32(2.0 * np.pi) * np.arange(q, dtype=np.float32)) / np.float32(r * q)
            twr, twi = np.cos(a32), np.sin(a32)
        conj = not inverse
        if bug == 'no_conj_%d' % r or (bug == 'no_conj_2' and r == 4):
            conj = False
        if conj:
            twi = -twi
        t = np.arange(G // r)
        j = t % q
        base = (t // q) * (r * q) + j
        at = [base + k * q for k in range(r)]
        wr, wi = twr[j][None, :], twi[j][None, :]
        if r == 4:
            w1r, w1i = (wr, wi) if bug == 'w1_is_w2' else _cmul(wr, wi, wr, wi)
            a = [(xr[:, i], xi[:, i]) for i in at]
            a1 = _cmul(w1r, w1i, *a[1])
            a3 = _cmul(w1r, w1i, *a[3])
            b0 = (a[0][0] + a1[0], a[0][1] + a1[1])
            b1 = (a[0][0] - a1[0], a[0][1] - a1[1])
            b2 = _cmul(wr, wi, a[2][0] + a3[0], a[2][1] + a3[1])
            t3 = _cmul(wr, wi, a[2][0] - a3[0], a[2][1] - a3[1])
            b3 = (-t3[1], t3[0]) if not conj else (t3[1], -t3[0])
            xr[:, at[0]], xi[:, at[0]] = b0[0] + b2[0], b0[1] + b2[1]
            xr[:, at[2]], xi[:, at[2]] = b0[0] - b2[0], b0[1] - b2[1]
            xr[:, at[1]], xi[:, at[1]] = b1[0] + b3[0], b1[1] + b3[1]
            xr[:, at[3]], xi[:, at[3]] = b1[0] - b3[0], b1[1] - b3[1]
        elif r == 2:
            a0 = (xr[:, at[0]], xi[:, at[0]])
            a1 = _cmul(wr, wi, xr[:, at[1]], xi[:, at[1]])
            xr[:, at[0]], xi[:, at[0]] = a0[0] + a1[0], a0[1] + a1[1]
            xr[:, at[1]], xi[:, at[1]] = a0[0] - a1[0], a0[1] - a1[1]
        else:
            rc, rs = roots[r]
            ins = []
            wkr, wki = None, None
            for k in range(r):
                v = (xr[:, at[k]], xi[:, at[k]])
                ins.append(_cmul(wkr, wki, *v) if k else v)
                wkr, wki = _cmul(wkr, wki, wr, wi) if k else (wr, wi)
            outs = []
            for c in range(r):
                accr, acci = ins[0]
                for k in range(1, r):
                    m = (k * c) % r
                    s = rs[m] if inverse else -rs[m]
                    pr, pi = _cmul(np.full((1, 1), rc[m], np.float32), np.full((1, 1), s, np.float32),
                                   *ins[k])
                    accr, acci = accr + pr, acci + pi
                outs.append((accr, acci))
            for c in range(r):
                xr[:, at[c]], xi[:, at[c]] = outs[c]
        q *= r
    out = xr.astype(np.float64) + 1j * xi.astype(np.float64)
    if bug == 'last_cell':
        out[:, G - 1] = 0.0
    return out


# ---------------------------------------------------------------------------------------------
# the bound

def _eta(r):
    return r * MU + (3 * r - 1) * U


@functools.lru_cache(maxsize=None)
def stage_constants(G):
    """(E, N) of the module docstring for one transform of G cells."""
    e = n = SECOND_ORDER
    for r in stages_of(G):
        if r == 4:
            a, b = 2 * MU + 5 * U, MU + 3 * U
            e *= 1 + a + b
            n *= (1 + math.sqrt(2.0) * a) * (1 + math.sqrt(2.0) * b)
        elif r == 2:
            e *= 1 + MU + 3 * U
            n *= 1 + math.sqrt(2.0) * (MU + 3 * U)
        else:
            e *= 1 + _eta(r)
            n *= 1 + math.sqrt(r) * _eta(r)
    return e - 1.0, n - 1.0


def transform_bound(op, G, norm):
    """The constant C (norm=False: per element, K included) or C' (norm=True) of the docstring
    for one entry point: multiply by the l1 (l2) norm the docstring names."""
    E, N = stage_constants(G)
    t = 1 + (N if norm else E)
    if op == 'beam':
        return (1 if norm else 4) * (t ** 4 * (1 + U) ** 2 * (1 + 6 * U) - 1)
    K = 1 if norm or op.endswith('_w') else 2
    if op.startswith('g2i'):
        c = (1 + U) ** 2 * t ** 2 * (1 + 3 * U)
        if op == 'g2i_w':
            c *= 1 + ROT
    else:
        c = (1 + 3 * U) * t ** 2 * (1 + U)
        if op == 'i2g_w':
            c *= 1 + 7 * U
    return K * (c - 1)


# ---------------------------------------------------------------------------------------------
# the Gg rule

HALVES = (511, 512, 513, 2047, 2048, 2049)
CATEGORIES = ('two', 'full', 'full_minus_2', 'production') + tuple('half_mod8_%d' % r for r in range(8)) \
    + tuple('half_%d' % h for h in HALVES)


POW2_CATEGORIES = ('full', 'full_minus_2', 'two', 'production', 'full', 'half_mod8_3', 'half_511',
                   'half_512', 'half_2047', 'full')


def grid_size_for(G, slot):
    """(Gg, category) for layer size G in `slot` (0: the real pair and the beam's turn, 1: the
    any-w pair): the categories in turn along the sorted sizes, the two slots half a cycle apart;
    a half the size cannot hold falls back to a seeded draw."""
    i = SIZES.index(G) + slot * (len(CATEGORIES) // 2)
    cat = CATEGORIES[i % len(CATEGORIES)]
    if G & (G - 1) == 0:        # the ten powers of two (kernels of their own) take a cycle of their own
        cat = POW2_CATEGORIES[(G.bit_length() - 5 + slot) % len(POW2_CATEGORIES)]
    if cat == 'two':
        return 2, cat
    if cat == 'full':
        return G, cat
    if cat == 'full_minus_2':
        return G - 2, cat
    if cat == 'production':
        return 2 * max(1, int(round(0.15 * G))), cat
    if cat.startswith('half_mod8_'):
        r = int(cat[-1])
        half = (G // 4) // 8 * 8 + r
        while half > G // 2:
            half -= 8
        if half >= 1:
            return 2 * half, cat
    else:
        half = int(cat[5:])
        if 2 * half <= G:
            return 2 * half, cat
    rs = np.random.RandomState(G * 2 + slot)
    return 2 * int(rs.randint(1, G // 2 + 1)), 'random'


# ---------------------------------------------------------------------------------------------
# the contract's float32 steps and the float64 truth, numpy

def _f32(v):
    return np.float32(v)


def correction32(G, kernel1d, lm_scale, lm_bias, w, xp=np):
    """n, t (float32) and r (float32 phase in turns, reduced) as the contract rounds them."""
    i = np.arange(G, dtype=np.float32)
    lm = i * _f32(lm_scale) + _f32(lm_bias)
    l2 = lm * lm
    n = np.sqrt(_f32(1.0) - (l2[:, None] + l2[None, :]))
    k = np.asarray(kernel1d, np.float32)
    t = k[:, None] * k[None, :]
    p = _f32(w) * (n - _f32(1.0))
    return n, t, p - np.rint(p)


def beam_factor(G, amplitude, a, b, c):
    """fl-steps of the beam's power in float32, the factor in float64: (G, G/2 + 1)."""
    ly = np.arange(G)
    v = np.where(2 * ly >= G, ly - G, ly).astype(np.float32)[:, None]
    u = np.arange(G // 2 + 1, dtype=np.float32)[None, :]
    a, b, c = _f32(a), _f32(b), _f32(c)
    power = (a * v + b * u) * v + (c * u) * u
    return float(_f32(amplitude)) * np.exp(power.astype(np.float64))


def transform_truth64(op, G, Gg=None, grid=None, image=None, kernel1d=None, lm_scale=0.0,
                      lm_bias=0.0, w=0.0, beam=None):
    """float64 truth of one entry point (numpy).  Returns (result, scale): scale is what the
    per-element bound multiplies (an array or a number), see the docstring."""
    hG = G // 2
    if op == 'beam':
        x = np.asarray(image, np.float64)
        B = beam_factor(G, *beam)
        Y = np.fft.ifft(np.fft.rfft2(x) * B, axis=0) * G
        Y[:, 0] = Y[:, 0].real
        Y[:, hG] = Y[:, hG].real
        return np.fft.irfft(Y, n=G, axis=1) * G, B.max() * G * G
    n, t, r = correction32(G, kernel1d, lm_scale, lm_bias, 0.0 if op.endswith('real') else w)
    n, t, r = n.astype(np.float64), t.astype(np.float64), r.astype(np.float64)
    half = Gg // 2
    if op.startswith('g2i'):
        big = np.zeros((G, G), np.complex128)
        big[hG - half:hG + half, hG - half:hG + half] = grid
        F = np.fft.fftshift(np.fft.ifft2(np.fft.ifftshift(big))) * (G * G)
        v = F.real * np.cos(2 * np.pi * r) - F.imag * np.sin(2 * np.pi * r)
        return v * n / t, n / t
    V = np.asarray(image, np.float64) / (t * n) * np.exp(-2j * np.pi * r)
    L = np.fft.fftshift(np.fft.fft2(np.fft.ifftshift(V)))
    return L[hG - half:hG + half, hG - half:hG + half], np.abs(V)


# ---------------------------------------------------------------------------------------------
# float64 restatement of the kernels' structure (for the simulated bugs only)

STRUCTURE_BUGS = ('pair_nyquist', 'fold_drops_column', 'shift_off_by_one', 'xcd_loses_block',
                  'beam_no_1_over_hw')


def xcd_contiguous(block, blocks, bug=None):
    xcd, each, extra = block % 8, blocks // 8, blocks % 8
    if bug == 'xcd_loses_block' and extra:
        return min(xcd * each + min(xcd, extra) + block // 8, blocks - 2)
    return xcd * each + min(xcd, extra) + block // 8


def structure_g2i_real(G, grid, bug=None):
    """g2i_columns_kernel + g2i_rows_kernel in float64 (transforms by numpy): the uncorrected
    image Re F, image-indexed."""
    Gg = grid.shape[0]
    half, hG = Gg // 2, G // 2
    big = np.zeros((G, G), np.complex128)
    idx = (np.arange(Gg) - half) % G
    big[np.ix_(idx, idx)] = grid
    if bug == 'fold_drops_column' and Gg == G:
        big[:, hG] = 0
    mirror = np.conj(big[(-np.arange(G)) % G][:, (-np.arange(G)) % G])
    hl = 0.5 * (big + mirror)[:, :half + 1]
    if bug == 'fold_drops_column' and Gg < G:
        hl[:, half] = 0         # (the column -half reaches only as the mirror of +half)
    T = np.fft.ifft(hl, axis=0).T * G                   # T[lx][sy]
    image = np.zeros((G, G))
    shift = (lambda i: (i + hG) % G)
    if bug == 'shift_off_by_one' and hG % 2:
        shift = (lambda i: (i + hG + 1) % G)
    for blk in range(G // 2):
        sy1 = 2 * xcd_contiguous(blk, G // 2, bug)
        x = np.zeros(G, np.complex128)
        for nn in range(half + 1):
            t1, t2 = T[nn][sy1], T[nn][sy1 + 1]
            nyq = (2 * nn == G) and bug != 'pair_nyquist'
            if nn == 0 or nyq:
                x[nn] = t1.real + 1j * t2.real
            else:
                x[nn] = t1 + 1j * t2
                x[(G - nn) % G] = np.conj(t1) + 1j * np.conj(t2)
        z = np.fft.ifft(x) * G
        image[shift(sy1)][shift(np.arange(G))] = z.real
        image[shift(sy1 + 1)][shift(np.arange(G))] = z.imag
    return image


# ---------------------------------------------------------------------------------------------
# inputs

def sparse_positions(size, seed):
    """DC, +-1, the extreme rows and columns, the corners and three seeded cells of a size^2
    array centred at size/2; {(row, col): complex value}, both parts non-zero."""
    h = size // 2
    rs = np.random.RandomState(seed)
    pos = [(h, h), (h, min(h + 1, size - 1)), (h - 1, h), (0, h), (size - 1, h), (h, 0), (h, size - 1),
           (0, 0), (size - 1, size - 1), (0, size - 1)]
    pos += [(int(rs.randint(size)), int(rs.randint(size))) for _ in range(3)]
    out = {}
    for p in pos:
        out[p] = complex(rs.uniform(0.5, 1.5) * rs.choice([-1, 1]), rs.uniform(0.5, 1.5) * rs.choice([-1, 1]))
    return out


def beam_coefficients(G, amplitude, sx, sy, theta):
    """FourierBeam.coefficients (beam.py) for a square image."""
    c, s = math.cos(theta), math.sin(theta)
    Q = np.array([[c, -s], [s, c]])
    M = Q @ np.diag([sx, sy]) @ Q.T
    amp = 2 * np.pi * amplitude * abs(np.linalg.det(M)) / (G * G)
    M = M @ np.diag([1.0 / G, 1.0 / G])
    C = -2 * np.pi ** 2 * M.T @ M
    return float(amp), float(C[0, 0]), float(2 * C[0, 1]), float(C[1, 1])


# ---------------------------------------------------------------------------------------------
# CPU tests

def test_sizes_and_refusals():
    """The library accepts exactly the 241 sizes of SIZES and refuses the issue's list."""
    from katsdpimager_amd._lib import lib
    L = lib()
    got = [G for G in range(2, 8300) if L.kimg_grid_image_real_supported(G, 2)]
    assert got == list(SIZES) and len(got) == 241
    for G, Gg in REFUSED:
        assert not L.kimg_grid_image_real_supported(G, Gg), (G, Gg)
        assert L.kimg_grid_image_real_workspace_bytes(G, Gg) == 0
        assert L.kimg_grid_image_w_workspace_bytes(G, Gg) == 0
    for G in (16, 4374, 8192):
        assert L.kimg_grid_image_real_workspace_bytes(G, G - 2) == 8 * (G // 2) * G
        assert L.kimg_grid_image_w_workspace_bytes(G, G - 2) == 8 * (G - 2) * G
    for G in REPRESENTATIVE + (4374, 4802, 6250, 18, 20, 28, 8100, 5832, 6720):
        assert G in SIZES


def test_grid_size_rule_covers_every_branch():
    """Over the sweep the Gg rule hits every category, every residue of Gg/2 + 1 and of Gg mod 8,
    Gg = G on both kernel instantiations, and each of the halves around the 512- and 2048-thread
    rounds."""
    seen, halves, columns, residues, full = set(), set(), set(), set(), set()
    for G in SIZES:
        for slot in (0, 1):
            Gg, cat = grid_size_for(G, slot)
            assert supported(G, Gg)
            seen.add((slot, cat))
            halves.add((slot, Gg // 2))
            columns.add((slot, (Gg // 2 + 1) % 8))
            residues.add((slot, Gg % 8))
            if Gg == G:
                full.add((slot, G & (G - 1) == 0))
    for slot in (0, 1):
        assert {c for s, c in seen if s == slot} >= set(CATEGORIES)
        assert {h for s, h in halves if s == slot} >= set(HALVES)
        assert {c for s, c in columns if s == slot} == set(range(8))
        assert {r for s, r in residues if s == slot} == {0, 2, 4, 6}
        assert {p for s, p in full if s == slot} == {False, True}
    assert {(G // 2) % 8 for G in SIZES} == set(range(8))       # row blocks: xcd_contiguous


def _model_inputs(G, seed):
    rs = np.random.RandomState(seed)
    dense = rs.standard_normal((2, G)) + 1j * rs.standard_normal((2, G))
    sparse = np.zeros((2, G), np.complex128)
    for row in range(2):
        for n in (0, 1, G // 2, G - 1, int(rs.randint(G)), int(rs.randint(G))):
            sparse[row, n] = complex(rs.uniform(0.5, 1.5), -rs.uniform(0.5, 1.5))
    return np.concatenate((dense, sparse)).astype(np.complex64)


def model_ratios(G, inverse, bug=None, seed=0):
    """(largest per-element ratio over the sparse rows, largest norm-wise ratio over the dense
    rows) of the float32 model against numpy's complex128 transform."""
    x = _model_inputs(G, seed + G)
    got = lds_fft_model(x, inverse, bug)
    x64 = x.astype(np.complex128)
    want = np.fft.ifft(x64, axis=1) * G if inverse else np.fft.fft(x64, axis=1)
    E, N = stage_constants(G)
    dev = np.abs(got - want)
    elem = (dev[2:].max(axis=1) / (E * np.abs(x64[2:]).sum(axis=1))).max()
    norm = (np.sqrt((dev[:2] ** 2).sum(axis=1)) / (N * np.sqrt((np.abs(want[:2]) ** 2).sum(axis=1)))).max()
    return float(elem), float(norm)




def test_model_within_bound():
    """The float32 model of lds_fft stays inside E ||x||_1 per element and N ||y||_2 norm-wise at
    all 241 sizes, both directions."""
    for inverse in (False, True):
        worst_e, worst_n = (0.0, 0), (0.0, 0)
        for G in SIZES:
            e, n = model_ratios(G, inverse)
            assert e < 1.0 and n < 1.0, (G, inverse, e, n)
            worst_e, worst_n = max(worst_e, (e, G)), max(worst_n, (n, G))
        print('model inverse=%s: per element %.3f at %d, norm %.3f at %d' % ((inverse,) + worst_e + worst_n))
        assert abs(worst_e[0] - MODEL[inverse][0]) < 0.005 and abs(worst_n[0] - MODEL[inverse][2]) < 0.005


def test_model_is_a_transform_of_small_integers_exactly():
    """A single non-zero cell at index 0 comes out as a constant bit for bit at every size: the
    premise of the exact GPU cases."""
    for G in SIZES:
        x = np.zeros((1, G), np.complex64)
        x[0, 0] = 3 + 5j
        for inverse in (False, True):
            assert np.all(lds_fft_model(x, inverse) == 3 + 5j), G


# bugs whose deviation / bound exceeds 1 wherever they act
SEEN = ('w1_is_w2', 'perm_swapped', 'last_cell', 'no_conj_2', 'no_conj_3', 'no_conj_5', 'no_conj_7')
# under the worst-case bound everywhere: the module cannot see them
BELOW_BOUND = ('twiddle_4ulp', 'table_float32', 'root5_digits', 'root7_digits')
# the 17-digit literals less their last decimal round to the same float32: not a bug at all
NO_CHANGE = ('root5_literal', 'root7_literal')
BUG_SIZES = SIZES


def test_truth_sees_simulated_bugs():
    """1-D bugs in the float32 model: deviation / bound over 1 wherever the bug can act (SEEN), or
    recorded as invisible (BELOW_BOUND, NO_CHANGE)."""
    for bug in MODEL_BUGS:
        smallest, largest = (np.inf, 0), (0.0, 0)
        for G in BUG_SIZES:
            for inverse in (False, True):
                if not bug_acts(bug, G, inverse):
                    continue
                ratio = max(model_ratios(G, inverse, bug))
                smallest, largest = min(smallest, (ratio, G)), max(largest, (ratio, G))
                if bug in SEEN:
                    assert ratio > 1.0, (bug, G, inverse, ratio)
        print('bug %-14s ratio %.3g (at %d) .. %.3g (at %d)' % ((bug,) + smallest + largest))
        if bug in BELOW_BOUND:
            assert largest[0] < 1.0, (bug, largest)
        if bug in NO_CHANGE:
            x = _model_inputs(70, 1)
            assert np.array_equal(lds_fft_model(x, True, bug), lds_fft_model(x, True))


def test_truth_sees_structure_bugs():
    """Bugs of the kernels' structure (pairing, fold, shift, block order, beam amplitude) in the
    float64 restatement: far over the bound where they act; the restatement itself equals the
    truth to float64 rounding."""
    rs = np.random.RandomState(3)
    for G, Gg in ((16, 16), (18, 18), (20, 6), (36, 36), (50, 50), (42, 20), (28, 28), (126, 126),
                  (120, 40), (140, 140)):
        grid = rs.standard_normal((Gg, Gg)) + 1j * rs.standard_normal((Gg, Gg))
        k = np.ones(G, np.float32)
        want, _ = transform_truth64('g2i_real', G, Gg, grid=grid, kernel1d=k)
        norm = np.sqrt((want ** 2).sum())
        assert np.sqrt(((structure_g2i_real(G, grid) - want) ** 2).sum()) < 1e-12 * norm
        bound = transform_bound('g2i_real', G, True) * norm
        for bug in STRUCTURE_BUGS[:4]:
            # (pair_nyquist: column G/2 of T is real up to rounding, so pairing it like the others
            # writes the same cell twice with the same value: no bug in exact arithmetic)
            acts = {'pair_nyquist': False, 'fold_drops_column': True,
                    'shift_off_by_one': (G // 2) % 2 == 1, 'xcd_loses_block': (G // 2) % 8 != 0}[bug]
            dev = np.sqrt(((structure_g2i_real(G, grid, bug) - want) ** 2).sum())
            if acts:
                assert dev / bound > 1e3, (bug, G, Gg, dev / bound)
            else:
                assert dev / bound < 1e-3, (bug, G, Gg)
    # the beam without 1 / (H W): off by G^2
    G = 36
    x = rs.uniform(-1, 1, (G, G))
    amp, a, b, c = beam_coefficients(G, 1.7, 2.3, 1.4, 0.5)
    want, scale = transform_truth64('beam', G, image=x, beam=(amp, a, b, c))
    wrong, _ = transform_truth64('beam', G, image=x, beam=(amp * G * G, a, b, c))
    bound = transform_bound('beam', G, True) * scale * np.sqrt((x ** 2).sum())
    assert np.sqrt(((wrong - want) ** 2).sum()) / bound > 1e3


def test_truth_is_the_oracle_at_small_sizes():
    """transform_truth64 agrees with the all-float64 oracle route (helpers.grid_to_image_truth) up to
    the float32 steps the contract fixes: 4e-7 |w| + 1e-6 of the peak."""
    from helpers import grid_to_image_truth
    rs = np.random.RandomState(11)
    G, Gg = 48, 20
    grid = rs.standard_normal((Gg, Gg)) + 1j * rs.standard_normal((Gg, Gg))
    k = rs.uniform(0.5, 2.0, G).astype(np.float32)
    scale, bias = 0.9 / G, -0.45
    for w in (0.0, 3.5):
        full = np.zeros((1, G, G), np.complex128)
        full[0, G // 2 - Gg // 2:G // 2 + Gg // 2, G // 2 - Gg // 2:G // 2 + Gg // 2] = grid
        want = grid_to_image_truth(full, k, np.float32(scale), np.float32(bias), w)[0]
        got, _ = transform_truth64('g2i_w', G, Gg, grid=grid, kernel1d=k, lm_scale=scale, lm_bias=bias, w=w)
        assert np.abs(got - want).max() < (4e-7 * abs(w) * 2 * np.pi + 1e-6) * np.abs(want).max()


# ---------------------------------------------------------------------------------------------
# GPU: buffers and calls through the C ABI

gpu = pytest.mark.gpu
SENTINEL = 1.5e30
GUARD = 64      # elements in front of and behind every buffer


def _torch():
    import torch
    return torch


def _stream():
    return _torch().cuda.current_stream().cuda_stream


class Padded:
    """rows x width cells of `dtype` with row stride `stride`, GUARD cells in front and behind,
    everything outside the payload a sentinel; .view is the payload, .untouched() whether all the
    rest still holds the sentinel."""
    def __init__(self, rows, width, dtype, stride=None, value=None):
        torch = _torch()
        self.stride = stride or width
        self.flat = torch.full((2 * GUARD + rows * self.stride,), SENTINEL, dtype=dtype, device='cuda')
        self.view = self.flat[GUARD:GUARD + rows * self.stride].view(rows, self.stride)[:, :width]
        if value is not None:
            self.view.copy_(value)
        self.rows, self.width = rows, width

    @property
    def ptr(self):
        return self.view.data_ptr()

    def untouched(self):
        body = self.flat[GUARD:GUARD + self.rows * self.stride].view(self.rows, self.stride)
        return bool((self.flat[:GUARD] == SENTINEL).all() and (self.flat[-GUARD:] == SENTINEL).all()
                    and (body[:, self.width:] == SENTINEL).all())


class Workspace:
    """Exactly `nbytes` bytes, 16-byte aligned, with a sentinel guard behind."""
    def __init__(self, nbytes):
        torch = _torch()
        self.nbytes = nbytes
        self.flat = torch.full((nbytes // 4 + GUARD,), SENTINEL, dtype=torch.float32, device='cuda')
        assert self.flat.data_ptr() % 16 == 0 and nbytes % 16 == 0
        self.ptr = self.flat.data_ptr()

    def untouched(self):
        return bool((self.flat[self.nbytes // 4:] == SENTINEL).all())


def workspace_bytes(op, G, Gg):
    from katsdpimager_amd._lib import lib
    if op == 'beam':
        return 8 * (G // 2 + 1) * G
    fn = lib().kimg_grid_image_w_workspace_bytes if op.endswith('_w') else lib().kimg_grid_image_real_workspace_bytes
    return fn(G, Gg)


def call(op, G, Gg=None, grid=None, image=None, k1d=None, lm_scale=0.0, lm_bias=0.0, w=0.0,
         accumulate=0, beam=None, ws=None, ws_bytes=None, stream=None):
    """One entry point on Padded buffers; returns the status code."""
    from katsdpimager_amd._lib import lib
    L = lib()
    ws = ws or Workspace(workspace_bytes(op, G, Gg))
    nbytes = ws.nbytes if ws_bytes is None else ws_bytes
    s = _stream() if stream is None else stream
    if op == 'beam':
        return L.kimg_convolve_beam(image.ptr, image.stride, G, *beam, ws.ptr, nbytes, s)
    if op == 'g2i_real':
        return L.kimg_grid_to_image_real(image.ptr, image.stride, G, grid.ptr, grid.stride, Gg, k1d.data_ptr(),
                                         lm_scale, lm_bias, accumulate, ws.ptr, nbytes, s)
    if op == 'g2i_w':
        return L.kimg_grid_to_image_w(image.ptr, image.stride, G, grid.ptr, grid.stride, Gg, k1d.data_ptr(),
                                      lm_scale, lm_bias, w, accumulate, ws.ptr, nbytes, s)
    if op == 'i2g_real':
        return L.kimg_image_to_grid_real(grid.ptr, grid.stride, Gg, image.ptr, image.stride, G, k1d.data_ptr(),
                                         lm_scale, lm_bias, ws.ptr, nbytes, s)
    return L.kimg_image_to_grid_w(grid.ptr, grid.stride, Gg, image.ptr, image.stride, G, k1d.data_ptr(),
                                  lm_scale, lm_bias, w, ws.ptr, nbytes, s)


# ---------------------------------------------------------------------------------------------
# GPU: the truth on the device (float32 steps in eager float32 torch, the rest in float64)

def correction_dev(G, k1d, lm_scale, lm_bias, w):
    torch = _torch()
    i = torch.arange(G, dtype=torch.float32, device='cuda')
    lm = i * float(np.float32(lm_scale))
    lm = lm + float(np.float32(lm_bias))
    l2 = lm * lm
    s = l2[:, None] + l2[None, :]
    n = torch.sqrt(1.0 - s)
    t = k1d[:, None] * k1d[None, :]
    p = (n - 1.0) * float(np.float32(w))
    return n, t, p - torch.round(p)


def _phase_vectors(freq, index, G, sign):
    """exp(sign 2 pi i freq[k] index[j] / G), (K, J) complex128, the angle reduced in integers."""
    torch = _torch()
    prod = (freq[:, None].to(torch.int64) * index[None, :].to(torch.int64)) % G
    ang = prod.to(torch.float64) * (sign * 2.0 * math.pi / G)
    return torch.complex(torch.cos(ang), torch.sin(ang))


def truth_dev(op, G, Gg=None, grid=None, image=None, k1d=None, lm_scale=0.0, lm_bias=0.0, w=0.0,
              beam=None, sparse=None, fft=False):
    """transform_truth64 on the device.  Dense inputs: the 2-D sums as complex128 matrix products
    with exact-angle phase matrices (the BLAS library; no FFT plan per size), or with fft=True
    torch.fft in complex128.  grid / image: torch tensors (payload views).  sparse: the
    {(row, col): value} the input was made from -> closed form instead of an FFT.  Returns
    (truth, elem_scale, norm_scale): per-element bounds multiply elem_scale ||input||_1-like,
    see _check."""
    torch = _torch()
    hG = G // 2
    c128 = torch.complex128
    if op == 'beam':
        x = image.to(torch.float64)
        ly = torch.arange(G, device='cuda')
        v = torch.where(2 * ly >= G, ly - G, ly).to(torch.float32)[:, None]
        u = torch.arange(hG + 1, dtype=torch.float32, device='cuda')[None, :]
        amp, a, b, c = (float(np.float32(z)) for z in beam)
        power = (v * a + u * b) * v + (u * c) * u
        B = amp * torch.exp(power.to(torch.float64))
        if fft:
            Y = torch.fft.ifft(torch.fft.rfft2(x) * B, dim=0, norm='forward')
        else:
            ar = torch.arange(G, device='cuda')
            W = _phase_vectors(ar, ar, G, -1)
            Y = W.conj() @ ((W @ x.to(c128) @ W[:, :hG + 1]) * B)
        Y[:, 0] = Y[:, 0].real.to(c128)
        Y[:, hG] = Y[:, hG].real.to(c128)
        if fft:
            out = torch.fft.irfft(Y, n=G, dim=1, norm='forward')
        else:       # the complex-to-real sum: columns 1 .. G/2 - 1 count twice
            Y[:, 1:hG] *= 2.0
            out = (Y @ W[:hG + 1, :].conj()).real
            del W
        Bmax = float(B.max())
        return out, Bmax * G * G * float(x.abs().sum()), Bmax * G * G * float(torch.linalg.norm(x))
    n, t, r = correction_dev(G, k1d, lm_scale, lm_bias, 0.0 if op.endswith('real') else w)
    n, t, r = n.to(torch.float64), t.to(torch.float64), r.to(torch.float64)
    half = Gg // 2
    if op.startswith('g2i'):
        if sparse is not None:
            keys = list(sparse)
            cy = torch.tensor([p[0] - half for p in keys], device='cuda')
            cx = torch.tensor([p[1] - half for p in keys], device='cuda')
            val = torch.tensor([sparse[p] for p in keys], dtype=c128, device='cuda')
            idx = torch.arange(G, device='cuda') - hG       # image index y <-> centred coordinate
            F = (_phase_vectors(cy, idx, G, 1) * val[:, None]).T @ _phase_vectors(cx, idx, G, 1)
        elif not fft:
            A = _phase_vectors(torch.arange(Gg, device='cuda') - half, torch.arange(G, device='cuda') - hG, G, 1)
            F = A.T @ grid.to(c128) @ A
            del A
        else:
            big = torch.zeros((G, G), dtype=c128, device='cuda')
            big[hG - half:hG + half, hG - half:hG + half] = grid.to(c128)
            F = torch.fft.fftshift(torch.fft.ifft2(torch.fft.ifftshift(big), norm='forward'))
            del big
        ang = 2.0 * math.pi * r
        v = F.real * torch.cos(ang) - F.imag * torch.sin(ang)
        corr = n / t
        return (v * corr, corr * float(grid.abs().to(torch.float64).sum()),
                float(torch.linalg.norm(F)) if op == 'g2i_w' else float(torch.linalg.norm(F.real)))
    ang = -2.0 * math.pi * r
    mag = image.to(torch.float64) / (t * n)
    if sparse is not None:
        keys = list(sparse)
        ys = torch.tensor([p[0] for p in keys], device='cuda')
        xs = torch.tensor([p[1] for p in keys], device='cuda')
        V = mag[ys, xs] * torch.complex(torch.cos(ang[ys, xs]), torch.sin(ang[ys, xs]))
        freq = torch.arange(Gg, device='cuda') - half
        out = (_phase_vectors(ys - hG, freq, G, -1) * V[:, None]).T @ _phase_vectors(xs - hG, freq, G, -1)
    elif not fft:
        V = mag * torch.complex(torch.cos(ang), torch.sin(ang))
        A = _phase_vectors(torch.arange(Gg, device='cuda') - half, torch.arange(G, device='cuda') - hG, G, -1)
        out = A @ V @ A.T
        del A, V
    else:
        V = mag * torch.complex(torch.cos(ang), torch.sin(ang))
        L = torch.fft.fftshift(torch.fft.fft2(torch.fft.ifftshift(V)))
        out = L[hG - half:hG + half, hG - half:hG + half].clone()
        del L, V
    return out, float(mag.abs().sum()), G * float(torch.linalg.norm(mag))


def ratios(op, G, got, truth, elem_scale, norm_scale, corr=None):
    """(per-element ratio, norm-wise ratio, peak-relative deviation).  corr: the n / t of
    grid -> image, by which the norm-wise comparison divides first."""
    torch = _torch()
    dev = (got.to(truth.dtype) - truth).abs()
    elem = float((dev / (transform_bound(op, G, False) * elem_scale)).max())
    weighted = dev if corr is None else dev / corr
    norm = float(torch.linalg.norm(weighted)) / (transform_bound(op, G, True) * norm_scale)
    return elem, norm, float(dev.max() / truth.abs().max())


def _inputs(op, G, Gg, dense, seed):
    """(grid Padded or None, image Padded, sparse dict or None) for one case."""
    torch = _torch()
    gen = torch.Generator(device='cuda').manual_seed(seed)
    grid = sparse = None
    if op.startswith('g2i'):
        if dense:
            g = torch.complex(torch.randn((Gg, Gg), generator=gen, device='cuda'),
                              torch.randn((Gg, Gg), generator=gen, device='cuda'))
        else:
            sparse = sparse_positions(Gg, seed)
            host = np.zeros((Gg, Gg), np.complex64)
            for (y, x), v in sparse.items():
                host[y, x] = v
            g = torch.from_numpy(host).cuda()
            sparse = {p: complex(np.complex64(v)) for p, v in sparse.items()}
        grid = Padded(Gg, Gg, torch.complex64, value=g)
        image = Padded(G, G, torch.float32, value=torch.zeros((G, G), device='cuda'))
    else:
        if dense:
            m = torch.rand((G, G), generator=gen, device='cuda') * 2 - 1
        else:
            sparse = {p: float(np.float32(v.real)) for p, v in sparse_positions(G, seed).items()}
            host = np.zeros((G, G), np.float32)
            for (y, x), v in sparse.items():
                host[y, x] = v
            m = torch.from_numpy(host).cuda()
        image = Padded(G, G, torch.float32, value=m)
        if op != 'beam':
            grid = Padded(Gg, Gg, torch.complex64, value=torch.zeros((Gg, Gg), dtype=torch.complex64, device='cuda'))
            if dense:
                sparse = None
    return grid, image, sparse


def run_case(op, G, Gg, dense, seed, lm_scale=None, lm_bias=None, w=0.0, beam=None, k1d=None):
    """One call with a fresh, exactly sized, guarded workspace against the device truth:
    (per-element ratio, norm ratio, peak-relative deviation)."""
    torch = _torch()
    lm_scale = 0.9 / G if lm_scale is None else lm_scale
    lm_bias = -0.5 * G * lm_scale if lm_bias is None else lm_bias
    if k1d is None:
        gen = torch.Generator(device='cuda').manual_seed(G)
        k1d = torch.rand((G,), generator=gen, device='cuda') * 1.5 + 0.5
    if op == 'beam' and beam is None:
        beam = beam_coefficients(G, 1.7, 2.3, 1.4, 0.5)
    grid, image, sparse = _inputs(op, G, Gg, dense, seed)
    ws = Workspace(workspace_bytes(op, G, Gg))
    kw = dict(k1d=k1d, lm_scale=lm_scale, lm_bias=lm_bias, w=w, beam=beam)
    if op == 'beam' and sparse is not None:
        sparse = None           # (the beam's truth is an FFT either way; sparse input, per-element bound)
    src = image.view.clone() if op == 'beam' else None
    truth, es, ns = truth_dev(op, G, Gg, grid=grid.view if grid else None,
                              image=src if op == 'beam' else image.view, sparse=sparse, **kw)
    rc = call(op, G, Gg, grid=grid, image=image, ws=ws, **kw)
    assert rc == 0, (op, G, Gg, rc)
    torch.cuda.synchronize()
    assert ws.untouched() and image.untouched() and (grid is None or grid.untouched()), (op, G, Gg)
    got = grid.view if op.startswith('i2g') else image.view
    corr = None
    if op.startswith('g2i'):
        n, t, _ = correction_dev(G, k1d, lm_scale, lm_bias, 0.0)
        corr = n.to(torch.float64) / t.to(torch.float64)
    return ratios(op, G, got, truth, es, ns, corr)


PEAK_LIMIT = 2e-6       # the coarse third assertion: own transform against truth, of the peak


WORST = {}      # (op, 'element' | 'norm' | 'peak') -> (largest ratio, size), filled as the cases run
CASES_RUN = set()


def _assert_case(op, G, Gg, dense, res):
    elem, norm, peak = res
    CASES_RUN.add((op, G, dense))
    for key, value in ((('element', elem),) if not dense else (('norm', norm), ('peak', peak))):
        WORST[(op, key)] = max(WORST.get((op, key), (0.0, 0)), (value, G))
    print('ratio %s G=%d Gg=%s %s: element %.4f norm %.4f peak %.2e'
          % (op, G, Gg, 'dense' if dense else 'sparse', elem, norm, peak))
    if dense:
        assert norm < 1.0, (op, G, Gg, norm)
        assert peak < PEAK_LIMIT, (op, G, Gg, peak)
    else:
        assert elem < 1.0, (op, G, Gg, elem)


@gpu
def test_device_float32_steps_match_numpy():
    """The eager float32 steps of correction_dev equal numpy's bit for bit (n, t, r), and so does
    the beam's power: the device truth rounds where the contract rounds."""
    torch = _torch()
    for G, w in ((250, 117.25), (1024, -12345.5)):
        k = np.random.RandomState(G).uniform(0.5, 2.0, G).astype(np.float32)
        scale, bias = 0.9 / G, -0.45
        want = correction32(G, k, scale, bias, w)
        got = correction_dev(G, torch.from_numpy(k).cuda(), scale, bias, w)
        for a, b in zip(want, got):
            assert np.array_equal(a, b.cpu().numpy())


@gpu
@pytest.mark.parametrize('G', (16, 70, 486))
def test_device_truth_agrees_with_numpy_and_closed_form(G):
    """truth_dev (torch.fft, float64) against transform_truth64 (numpy) and against the closed
    form of sparse inputs, all five operations: 1e-12 of the peak."""
    torch = _torch()
    Gg = grid_size_for(G, 0)[0]
    k = np.random.RandomState(G).uniform(0.5, 2.0, G).astype(np.float32)
    kd = torch.from_numpy(k).cuda()
    scale, bias, w = 0.9 / G, -0.45, 17.25
    for op in OPS:
        for dense in (True, False):
            grid, image, sparse = _inputs(op, G, Gg, dense, 7)
            beam = beam_coefficients(G, 1.7, 2.3, 1.4, 0.5)
            kw = dict(lm_scale=scale, lm_bias=bias, w=w, beam=beam)
            gv = grid.view if grid else None
            fft = truth_dev(op, G, Gg, grid=gv, image=image.view, k1d=kd, fft=True, **kw)[0].cpu().numpy()
            mat = truth_dev(op, G, Gg, grid=gv, image=image.view, k1d=kd, **kw)[0].cpu().numpy()
            assert np.abs(mat - fft).max() < 1e-12 * np.abs(fft).max(), (op, dense)
            host = transform_truth64(op, G, Gg, grid=None if gv is None else gv.cpu().numpy(),
                                     image=image.view.cpu().numpy(), kernel1d=k, **kw)[0]
            assert np.abs(fft - host).max() < 1e-12 * np.abs(host).max(), (op, dense)
            if sparse is not None and op != 'beam':
                closed = truth_dev(op, G, Gg, grid=gv, image=image.view, k1d=kd, sparse=sparse, **kw)[0]
                assert np.abs(closed.cpu().numpy() - host).max() < 1e-12 * np.abs(host).max(), op


@gpu
def test_closed_form_at_the_largest_size():
    """At 8192 the matrix-product and the FFT truth of a sparse grid equal the closed form to 1e-11
    of the peak."""
    torch = _torch()
    G, Gg = 8192, 2458
    kd = torch.ones(G, device='cuda')
    grid, image, sparse = _inputs('g2i_w', G, Gg, False, 5)
    kw = dict(grid=grid.view, image=image.view, k1d=kd, lm_scale=0.9 / G, lm_bias=-0.45, w=117.25)
    b = truth_dev('g2i_w', G, Gg, sparse=sparse, **kw)[0]
    for fft in (False, True):
        a = truth_dev('g2i_w', G, Gg, fft=fft, **kw)[0]
        assert float((a - b).abs().max() / b.abs().max()) < 1e-11, fft


ORDER = (8192, 16, 5832, 6720, 8192)
ORDER_RESULTS = {}      # (op, G) -> result of the first call of the process, kept for the second test


def _order_problem(op, G):
    """One fixed problem per (op, G): (result buffer, everything to keep alive, call arguments)."""
    torch = _torch()
    Gg = grid_size_for(G, 0)[0]
    gen = torch.Generator(device='cuda').manual_seed(G)
    k1d = torch.rand((G,), generator=gen, device='cuda') * 1.5 + 0.5
    grid, image, _ = _inputs(op, G, Gg, True, G + 1)
    kw = dict(grid=grid, image=image, k1d=k1d, lm_scale=0.9 / G, lm_bias=-0.45, w=17.25,
              beam=beam_coefficients(G, 1.7, 2.3, 1.4, 0.5), ws=Workspace(workspace_bytes(op, G, Gg)))
    return (grid if op.startswith('i2g') else image), (op, G, Gg), kw


@gpu
def test_order_of_sizes_and_two_streams():
    """The first test of the file to launch a kernel of the library, so plans and LDS attributes
    start from nothing: large -> small -> above the 64 KB LDS crossing (5832) -> below it (6720)
    -> large again, all five entry points, both instantiations (8192 and 16 are powers of two).
    The second 8192 equals the first bit for bit, every result is inside the norm-wise bound, and
    test_order_results_equal_one_size_at_a_time compares them again at the end of the run.  Then two
    sizes, one of them new, on two streams with all calls issued back to back."""
    torch = _torch()
    for G in ORDER:
        for op in OPS:
            buf, (_, _, Gg), kw = _order_problem(op, G)
            src = kw['image'].view.clone()
            assert call(op, G, Gg, **kw) == 0
            torch.cuda.synchronize()
            if (op, G) in ORDER_RESULTS:
                assert torch.equal(buf.view, ORDER_RESULTS[(op, G)]), (op, G)
                continue
            ORDER_RESULTS[(op, G)] = buf.view.clone()
            tkw = {k: kw[k] for k in ('k1d', 'lm_scale', 'lm_bias', 'w', 'beam')}
            truth, es, ns = truth_dev(op, G, Gg, grid=kw['grid'].view if kw['grid'] else None, image=src, **tkw)
            corr = None
            if op.startswith('g2i'):
                n, t, _ = correction_dev(G, kw['k1d'], kw['lm_scale'], kw['lm_bias'], 0.0)
                corr = n.to(torch.float64) / t.to(torch.float64)
            res = ratios(op, G, buf.view, truth, es, ns, corr)
            assert res[1] < 1.0 and res[2] < PEAK_LIMIT, (op, G, res)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    problems = [(s, _order_problem(op, G)) for rep in range(2) for op in OPS
                for s, G in zip(streams, (6720, 1250))]
    torch.cuda.synchronize()        # inputs and sentinels were written on the default stream
    for s, (buf, (op, G, Gg), kw) in problems:
        assert call(op, G, Gg, stream=s.cuda_stream, **kw) == 0
    torch.cuda.synchronize()
    for s, (buf, (op, G, Gg), kw) in problems:
        assert kw['ws'].untouched() and buf.untouched()
        if (op, G) in ORDER_RESULTS:
            assert torch.equal(buf.view, ORDER_RESULTS[(op, G)]), (op, G)
        ORDER_RESULTS[(op, G)] = buf.view.clone()


@gpu
@pytest.mark.parametrize('G', SIZES)
def test_every_size_against_truth(G):
    """Every accepted layer size through all five entry points: sparse input per element, dense
    input norm-wise (and 2e-6 of the peak), the two exact cases; guards and the space behind an
    exactly sized workspace untouched."""
    torch = _torch()
    for op in OPS:
        Gg = G if op == 'beam' else grid_size_for(G, 1 if op.endswith('_w') else 0)[0]
        for dense in (False, True):
            res = run_case(op, G, Gg, dense, seed=G + dense, w=W_ALL_SIZES)
            _assert_case(op, G, Gg, dense, res)
    # exact: DC-only grid -> constant image; centre pixel -> constant grid
    ones = torch.ones(G, device='cuda')
    for op in ('g2i_real', 'g2i_w'):
        Gg = grid_size_for(G, 1 if op.endswith('_w') else 0)[0]
        g = torch.zeros((Gg, Gg), dtype=torch.complex64, device='cuda')
        g[Gg // 2, Gg // 2] = 3 + 5j
        grid = Padded(Gg, Gg, torch.complex64, value=g)
        for accumulate in (0, 1):
            image = Padded(G, G, torch.float32, value=torch.full((G, G), 7.0, device='cuda'))
            assert call(op, G, Gg, grid=grid, image=image, k1d=ones, w=W_ALL_SIZES, accumulate=accumulate) == 0
            assert bool((image.view == (10.0 if accumulate else 3.0)).all()), (op, G, Gg, accumulate)
            assert image.untouched()
    for op in ('i2g_real', 'i2g_w'):
        Gg = grid_size_for(G, 1 if op.endswith('_w') else 0)[0]
        m = torch.zeros((G, G), device='cuda')
        m[G // 2, G // 2] = 3.0
        image = Padded(G, G, torch.float32, value=m)
        grid = Padded(Gg, Gg, torch.complex64, value=torch.full((Gg, Gg), 9 - 4j, dtype=torch.complex64, device='cuda'))
        assert call(op, G, Gg, grid=grid, image=image, k1d=ones, w=W_ALL_SIZES) == 0
        assert bool((grid.view == 3.0).all()), (op, G, Gg)      # overwritten, not added to
        assert grid.untouched()


@gpu
@pytest.mark.parametrize('G', REPRESENTATIVE)
def test_w_bias_and_scale(G):
    """Off-centre lm_bias (-size/3), lm_scale up to where 1 - l^2 - m^2 is small at the corners,
    w small, +-O(100), +-O(10^4); w = 0 through the any-w pair agrees with the real pair inside
    the sum of both bounds."""
    torch = _torch()
    Gg = grid_size_for(G, 0)[0]
    cases = [(0.9 / G, None, 0.03), (0.9 / G, None, -113.5), (0.9 / G, None, 9876.25),
             (0.9 / G, None, -12345.5), (0.6 / G, -0.6 / 3, 117.25), (1.39 / G, None, 40.5)]
    for scale, bias, w in cases:
        for op in ('g2i_w', 'i2g_w'):
            for dense in ((False, True) if w in (0.03, -12345.5) else (True,)):
                res = run_case(op, G, Gg, dense, seed=G + 3, lm_scale=scale, lm_bias=bias, w=w)
                _assert_case(op, G, Gg, dense, res)
    for op in ('g2i_real', 'i2g_real'):
        res = run_case(op, G, Gg, True, seed=G + 4, lm_scale=0.6 / G, lm_bias=-0.6 / 3)
        _assert_case(op, G, Gg, True, res)
    # w = 0: both pairs, one input
    k1d = torch.rand((G,), device='cuda') * 1.5 + 0.5
    scale, bias = 0.9 / G, -0.45
    for pair in ('g2i', 'i2g'):
        out = []
        for op in (pair + '_real', pair + '_w'):
            grid, image, _ = _inputs(op, G, Gg, True, G)
            assert call(op, G, Gg, grid=grid, image=image, k1d=k1d, lm_scale=scale, lm_bias=bias, w=0.0) == 0
            out.append((grid.view if pair == 'i2g' else image.view).clone())
        truth, es, ns = truth_dev(pair + '_w', G, Gg, grid=grid.view, image=image.view, k1d=k1d,
                                  lm_scale=scale, lm_bias=bias, w=0.0)
        dev = (out[0] - out[1]).abs().to(torch.float64)
        if pair == 'g2i':
            n, t, _ = correction_dev(G, k1d, scale, bias, 0.0)
            dev = dev * t.to(torch.float64) / n.to(torch.float64)
        both = transform_bound(pair + '_real', G, True) + transform_bound(pair + '_w', G, True)
        assert float(torch.linalg.norm(dev)) < both * ns, (pair, G)


def _refused(op, G, Gg, grid, image, kw):
    """What kimg.h promises of every function: a workspace one byte short, a misaligned one, an
    image or grid stride below the width -> KIMG_EINVAL, and no buffer changes."""
    torch = _torch()
    before = [b.flat.clone() for b in (grid, image) if b is not None]
    nbytes = workspace_bytes(op, G, Gg)
    ws = Workspace(nbytes + 16)
    assert call(op, G, Gg, grid=grid, image=image, ws=ws, ws_bytes=nbytes - 1, **kw) == KIMG_EINVAL
    ws.ptr += 8
    assert call(op, G, Gg, grid=grid, image=image, ws=ws, ws_bytes=nbytes, **kw) == KIMG_EINVAL
    ws.ptr -= 8
    for b in (grid, image):
        if b is not None:
            stride, b.stride = b.stride, b.width - 1
            assert call(op, G, Gg, grid=grid, image=image, ws=ws, ws_bytes=nbytes, **kw) == KIMG_EINVAL
            b.stride = stride
    torch.cuda.synchronize()
    assert bool((ws.flat == SENTINEL).all())
    for b, old in zip([b for b in (grid, image) if b is not None], before):
        assert torch.equal(b.flat.view(torch.int32), old.view(torch.int32)), op


@gpu
@pytest.mark.parametrize('G', REPRESENTATIVE)
def test_strides_accumulate_and_workspace(G):
    """Padded strides with sentinels everywhere, accumulate 0 / 1 twice in a row onto a non-zero
    image, image -> grid onto a prefilled grid (overwritten), a workspace one byte short and a
    misaligned one refused with nothing written."""
    torch = _torch()
    Gg = grid_size_for(G, 1)[0]
    k1d = torch.rand((G,), device='cuda') * 1.5 + 0.5
    scale, bias, w = 0.9 / G, -0.45, 17.25
    kw = dict(k1d=k1d, lm_scale=scale, lm_bias=bias, w=w)
    g = torch.complex(torch.randn((Gg, Gg), device='cuda'), torch.randn((Gg, Gg), device='cuda'))
    m = torch.rand((G, G), device='cuda') * 2 - 1
    for op in ('g2i_real', 'g2i_w'):
        grid = Padded(Gg, Gg, torch.complex64, stride=Gg + 3, value=g)
        plain = Padded(G, G, torch.float32, value=torch.zeros((G, G), device='cuda'))
        assert call(op, G, Gg, grid=Padded(Gg, Gg, torch.complex64, value=g), image=plain, **kw) == 0
        image = Padded(G, G, torch.float32, stride=G + 5, value=m)
        ws = Workspace(workspace_bytes(op, G, Gg))
        assert call(op, G, Gg, grid=grid, image=image, accumulate=0, ws=ws, **kw) == 0
        assert torch.equal(image.view, plain.view), op          # strides change nothing, old image gone
        expect = image.view.clone()
        for _ in range(2):
            assert call(op, G, Gg, grid=grid, image=image, accumulate=1, ws=ws, **kw) == 0
            expect = expect + plain.view                        # one float32 addition per pixel
        assert torch.equal(image.view, expect), op
        assert image.untouched() and grid.untouched() and ws.untouched(), op
        _refused(op, G, Gg, grid, image, kw)
    for op in ('i2g_real', 'i2g_w'):
        image = Padded(G, G, torch.float32, stride=G + 5, value=m)
        plain = Padded(Gg, Gg, torch.complex64, value=torch.zeros((Gg, Gg), dtype=torch.complex64, device='cuda'))
        assert call(op, G, Gg, grid=plain, image=Padded(G, G, torch.float32, value=m), **kw) == 0
        grid = Padded(Gg, Gg, torch.complex64, stride=Gg + 3, value=g)       # prefilled
        ws = Workspace(workspace_bytes(op, G, Gg))
        for _ in range(2):
            assert call(op, G, Gg, grid=grid, image=image, ws=ws, **kw) == 0
            assert torch.equal(grid.view, plain.view), op
        assert image.untouched() and grid.untouched() and ws.untouched(), op
        _refused(op, G, Gg, grid, image, kw)
    beam = beam_coefficients(G, 1.7, 2.3, 1.4, 0.5)
    plain = Padded(G, G, torch.float32, value=m)
    assert call('beam', G, image=plain, beam=beam) == 0
    image = Padded(G, G, torch.float32, stride=G + 7, value=m)
    ws = Workspace(workspace_bytes('beam', G, G))
    assert call('beam', G, image=image, beam=beam, ws=ws) == 0
    assert torch.equal(image.view, plain.view) and image.untouched() and ws.untouched()
    _refused('beam', G, G, None, image, dict(beam=beam))


@gpu
@pytest.mark.parametrize('G', REPRESENTATIVE)
def test_beams(G):
    """Narrow (sub-pixel), wide (sigma = G / 8), rotated beams with amplitude != 1: dense input
    norm-wise, a delta per element; the wide beam on a delta is the periodic Gaussian."""
    torch = _torch()
    for amp, sx, sy, theta in ((0.7, 0.4, 0.3, 0.0), (2.5, G / 8.0, G / 8.0, 0.0), (1.7, G / 16.0, 1.2, 1.1)):
        beam = beam_coefficients(G, amp, sx, sy, theta)
        for dense in (False, True):
            res = run_case('beam', G, G, dense, seed=G + 9, beam=beam)
            _assert_case('beam', G, G, dense, res)
    # a delta at (y0, x0) under the wide beam: amp sum_k exp(-((y - y0 + k G)^2 + (x - x0 + j G)^2) / 2 sigma^2)
    amp, sigma, y0, x0 = 2.5, G / 8.0, G // 3, G - 2
    m = torch.zeros((G, G), device='cuda')
    m[y0, x0] = 1.0
    image = Padded(G, G, torch.float32, value=m)
    beam = beam_coefficients(G, amp, sigma, sigma, 0.0)
    truth, es, ns = truth_dev('beam', G, image=m, beam=beam)
    idx = torch.arange(G, dtype=torch.float64, device='cuda')
    def periodic(c):
        d = idx - c
        return sum(torch.exp(-(d + k * G) ** 2 / (2 * sigma ** 2)) for k in (-2, -1, 0, 1, 2))
    closed = amp * periodic(y0)[:, None] * periodic(x0)[None, :]
    # (the float32 a, c of the contract move the width by 2^-24: 1e-6 of the peak)
    assert float((truth - closed).abs().max()) < 1e-6 * amp
    assert call('beam', G, image=image, beam=beam) == 0
    assert float((image.view.to(torch.float64) - truth).abs().max()) < transform_bound('beam', G, False) * es


@gpu
def test_operators_reach_the_same_kernels():
    """P = 1 .. 4 through GridImageTemplate (overwrite_next, accumulate, the layer buffer as the
    workspace) and ConvolveBeamTemplate: bit for bit the direct call's result per polarization."""
    torch = _torch()
    from helpers import context_queue
    from katsdpimager_amd import image as kimage, beam as kbeam
    ctx, q = context_queue()
    for G, Gg in ((70, 22), (256, 256), (1250, 376)):
        scale, bias = 0.9 / G, -0.45
        for P in (1, 2, 3, 4):
            rs = np.random.RandomState(G + P)
            g = (rs.standard_normal((P, Gg, Gg)) + 1j * rs.standard_normal((P, Gg, Gg))).astype(np.complex64)
            m = rs.uniform(-1, 1, (P, G, G)).astype(np.float32)
            k = rs.uniform(0.5, 2.0, G).astype(np.float32)
            kd = torch.from_numpy(k).cuda()
            template = kimage.GridImageTemplate(ctx, np.float32)
            plan = template.make_fft_plan((G, G))
            g2i = template.instantiate_grid_to_image(q, (P, Gg, Gg), scale, bias, plan)
            g2i.ensure_all_bound()
            i2g = template.instantiate_image_to_grid(q, (P, Gg, Gg), scale, bias, plan)
            i2g.bind(layer=g2i.buffer('layer'), kernel1d=g2i.buffer('kernel1d'))
            i2g.ensure_all_bound()
            g2i.buffer('kernel1d').set(q, k)
            g2i.buffer('grid').set(q, g)
            i2g.buffer('image').set(q, m)
            for w in (0.0, 17.25):
                op = 'g2i_real' if w == 0 else 'g2i_w'
                g2i.set_w(w)
                i2g.set_w(w)
                g2i.buffer('image').set(q, m)
                g2i.overwrite_next = True
                g2i()
                first = g2i.buffer('image').get(q)
                g2i()                                   # accumulates
                second = g2i.buffer('image').get(q)
                i2g()
                back = i2g.buffer('grid').get(q)
                q.finish()
                for pol in range(P):
                    grid = Padded(Gg, Gg, torch.complex64, value=torch.from_numpy(g[pol]).cuda())
                    image = Padded(G, G, torch.float32, value=torch.from_numpy(m[pol]).cuda())
                    kw = dict(k1d=kd, lm_scale=scale, lm_bias=bias, w=w)
                    assert call(op, G, Gg, grid=grid, image=image, accumulate=0, **kw) == 0
                    assert np.array_equal(image.view.cpu().numpy(), first[pol]), (G, P, w, pol)
                    assert call(op, G, Gg, grid=grid, image=image, accumulate=1, **kw) == 0
                    assert np.array_equal(image.view.cpu().numpy(), second[pol]), (G, P, w, pol)
                    image = Padded(G, G, torch.float32, value=torch.from_numpy(m[pol]).cuda())
                    assert call('i2g' + op[3:], G, Gg, grid=grid, image=image, **kw) == 0
                    assert np.array_equal(grid.view.cpu().numpy(), back[pol]), (G, P, w, pol)
        b = kbeam.Beam(1.7, 2.3, 1.4, 0.5)
        conv = kbeam.ConvolveBeamTemplate(ctx, (G, G), np.float32).instantiate(q)
        conv.ensure_all_bound()
        conv.beam = b
        conv.buffer('image').set(q, m[0])
        conv()
        got = conv.buffer('image').get(q)
        q.finish()
        image = Padded(G, G, torch.float32, value=torch.from_numpy(m[0]).cuda())
        assert call('beam', G, image=image, beam=conv._fourier_beam.coefficients()) == 0
        assert np.array_equal(image.view.cpu().numpy(), got), G


LIBRARY_SIZES = (16, 70, 486, 1024, 1250, 686, 5040, 8192)


@gpu
@pytest.mark.parametrize('dense', (True, False))
@pytest.mark.parametrize('G', LIBRARY_SIZES)
def test_library_route_within_the_same_bounds(G, dense):
    """{'own_transform': False}: the FFT library's float32 route stays inside the bounds derived
    for the own transforms (they assume nothing rocFFT does not also do: float32 twiddles,
    butterflies of radix <= 7... its larger radices are covered by the factor the bounds have
    in hand), dense input, w = 0 and w != 0, and the beam."""
    torch = _torch()
    from helpers import context_queue
    from katsdpimager_amd import image as kimage, beam as kbeam
    ctx, q = context_queue()
    Gg = grid_size_for(G, 0)[0]
    scale, bias = 0.9 / G, -0.45
    rs = np.random.RandomState(G)
    g = _inputs('g2i_w', G, Gg, dense, G)[0].view.cpu().numpy()[None]
    m = _inputs('i2g_w', G, Gg, dense, G)[1].view.cpu().numpy()[None]
    k = rs.uniform(0.5, 2.0, G).astype(np.float32)
    kd = torch.from_numpy(k).cuda()
    which = 1 if dense else 0       # norm-wise for dense input, per element for sparse
    kind = 'dense' if dense else 'sparse'
    template = kimage.GridImageTemplate(ctx, np.float32, {'own_transform': False})
    plan = template.make_fft_plan((G, G))
    g2i = template.instantiate_grid_to_image(q, (1, Gg, Gg), scale, bias, plan)
    g2i.ensure_all_bound()
    i2g = template.instantiate_image_to_grid(q, (1, Gg, Gg), scale, bias, plan)
    i2g.bind(layer=g2i.buffer('layer'), kernel1d=g2i.buffer('kernel1d'))
    i2g.ensure_all_bound()
    g2i.buffer('kernel1d').set(q, k)
    g2i.buffer('grid').set(q, g)
    i2g.buffer('image').set(q, m)
    for w in (0.0, 17.25):
        sfx = '_real' if w == 0 else '_w'
        g2i.set_w(w)
        i2g.set_w(w)
        g2i.buffer('image').zero(q)
        g2i()
        i2g()
        got_i = torch.from_numpy(g2i.buffer('image').get(q)[0]).cuda()
        got_g = torch.from_numpy(i2g.buffer('grid').get(q)[0]).cuda()
        kw = dict(k1d=kd, lm_scale=scale, lm_bias=bias, w=w)
        truth, es, ns = truth_dev('g2i' + sfx, G, Gg, grid=torch.from_numpy(g[0]).cuda(), **kw)
        n, t, _ = correction_dev(G, kd, scale, bias, 0.0)
        res = ratios('g2i' + sfx, G, got_i, truth, es, ns, n.to(torch.float64) / t.to(torch.float64))
        print('library g2i%s G=%d %s: ratio %.4f peak %.2e' % (sfx, G, kind, res[which], res[2]))
        assert res[which] < 1.0
        truth, es, ns = truth_dev('i2g' + sfx, G, Gg, image=torch.from_numpy(m[0]).cuda(), **kw)
        res = ratios('i2g' + sfx, G, got_g, truth, es, ns)
        print('library i2g%s G=%d %s: ratio %.4f peak %.2e' % (sfx, G, kind, res[which], res[2]))
        assert res[which] < 1.0
    conv = kbeam.ConvolveBeamTemplate(ctx, (G, G), np.float32, tuning={'own_transform': False}).instantiate(q)
    conv.ensure_all_bound()
    conv.beam = kbeam.Beam(1.7, 2.3, 1.4, 0.5)
    conv.buffer('image').set(q, m[0])
    conv()
    got = torch.from_numpy(conv.buffer('image').get(q)).cuda()
    truth, es, ns = truth_dev('beam', G, image=torch.from_numpy(m[0]).cuda(),
                              beam=conv._fourier_beam.coefficients())
    res = ratios('beam', G, got, truth, es, ns)
    print('library beam G=%d %s: ratio %.4f peak %.2e' % (G, kind, res[which], res[2]))
    assert res[which] < 1.0


@gpu
def test_order_results_equal_one_size_at_a_time():
    """After every size has run (all plans cached, attributes at their largest): each problem of
    test_order_of_sizes_and_two_streams alone, synchronised, equals what the sequence gave."""
    torch = _torch()
    if not ORDER_RESULTS:
        pytest.fail('test_order_of_sizes_and_two_streams has not run in this process')
    for (op, G), want in sorted(ORDER_RESULTS.items()):
        buf, (_, _, Gg), kw = _order_problem(op, G)
        torch.cuda.synchronize()
        assert call(op, G, Gg, **kw) == 0
        torch.cuda.synchronize()
        assert torch.equal(buf.view, want), (op, G)


@gpu
def test_report_largest_ratios():
    """Last in the file: prints the largest deviation / bound per operation over everything that
    ran (the source of MEASURED) and, after a full run, checks that no size was left out."""
    for key in sorted(WORST):
        print('largest %s %s: %.4g at %d' % (key + WORST[key]))
    sizes_run = {G for op, G, dense in CASES_RUN}
    if sizes_run >= set(SIZES):
        for op in OPS:
            for dense in (False, True):
                assert {G for o, G, d in CASES_RUN if o == op and d == dense} >= set(SIZES), (op, dense)
        for (op, key), (value, G) in WORST.items():
            assert value < 1.0 if key != 'peak' else value < PEAK_LIMIT
