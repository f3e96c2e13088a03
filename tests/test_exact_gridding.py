"""Exact parity of the gridder and degridder on integer-valued inputs.

The other gridder tests use the real Kaiser-Bessel / W tables and compare through a tolerance
relative to the peak; for K >= 28 most of a footprint lies below that tolerance, so a kernel that
drops, duplicates or misplaces its outer taps passes them.  Here the kernel table, the
visibilities, the density weights and the degridder's grid and weights are small integers, and
every partial sum stays below 2^24: float32 arithmetic is then exact in any summation order, so
every variant and arithmetic form must equal a float64 truth bit for bit, float atomics included,
and any lost, doubled or misplaced contribution moves some cell by at least 1.

Inputs: kernel taps with Re, Im independent in +-{1..7} (never 0: a zero tap hides a dropped one);
visibilities in {-3..3} + i{-3..3}; density weights in {1, 2, 3}, varying by cell and polarization;
degridder weights in {1, 2, 3}, starting visibilities in {-20..20} + i{-20..20}, grid values in
{-4..4} + i{-4..4}.

Premise, asserted for every case: the float64 sum over all terms of a cell (gridder) or of a
visibility (degridder) of the product of the factors' |Re| + |Im| stays below 2^24.  That bounds
every partial sum and every intermediate real product of any summation order, so a case that
breaks exactness fails loudly instead of flaking.

KIMG_ARITH_SPLIT_FP16 keeps integers of up to 11 bits exact (grid_mfma.hip, degrid_mfma.hip).  The
table is scaled by S = 2^(13 - e_k), which puts its largest component (exponent e_k) in
[2^13, 2^14), and the samples (vis * density weight) by T = 2^-E, with E the exponent of the
largest sample component of the group that set the scale, so that every sample component times T
is below 2.  A tap of at most 11 bits times S is exact in fp16: hi = tap, lo = 0.  The gridder's
row operand (s T) conj(kv S) is formed exactly in float32 (2 * 2047^2 < 2^23) and split with
round to nearest (v_cvt_pk_f16_f32).  After a round-to-nearest split the remainder of an
integer of up to 23 bits is at most half an ulp of hi and a whole number of its lowest unit, so it
fits the 11 bits of lo: hi + lo holds the operand exactly.  The "22 bits" of include/kimg.h bound
the relative error for arbitrary reals; they are no limit for such integers.  Its components
stay at or below 2 (2^14 - 8)(2 - 2^-10) < 65504, so nothing overflows, and their smallest unit,
S T >= 2^-22, is a multiple of the smallest fp16 subnormal.  The column operand has lo = 0, so
the dropped lo * lo term is 0, and fp16 x fp16 products are exact in float32.  The degridder
splits its window (scaled by a power of two from its largest value) and its row taps the same
way.  test_split_fp16_keeps_11_bit_integers replays these splits in numpy at every pair of scales,
exhaustively at the largest.  The inputs here (taps <= 3 bits, samples <= 4 bits, grid values
<= 3 bits) are well inside that range.

Table placement: only "in LDS" against "in HBM" can be observed through the C ABI (the workspace
size: 256 bytes when every table is in LDS).  Doubled against single LDS rows, and for K > 32 the
diagonal blocks' placement, come from _grid_placement / _degrid_placement, which restate the
launchers' LDS arithmetic; the kernels do not confirm them.

Footprint contract: with bias = (K - 1) // 2 - G // 2, every record has 0 <= u - bias <= G - K and
the same for v; the window kernels' 32-wide windows may hang over the grid's edge, footprints
never.

CPU tests (no marker): the truth itself changes under every simulated bug listed in
MUTATIONS (on the inputs of every gridder case of up to 4 M terms), and the premise holds for
every case configured for the GPU.  GPU tests are marked one
by one."""
import functools
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from helpers import Padded, context_queue        # noqa: E402

EXACT = float(1 << 24)
WIN = 32                                # window of the MFMA kernels (grid_mfma.hip, degrid_mfma.hip)
KIMG_EUNSUPPORTED = -10002
GRID_FORMS = ('fp32', 'fp32_32x32', 'split_fp16')
DEGRID_FORMS = ('fp32', 'split_fp16')


# ---------------------------------------------------------------------------------------------
# inputs

def _slack(K):
    return WIN - (K if K <= WIN else (K + 1) // 2)


def _walk(rs, n, M, track=512, start=None):
    """Slow tracks: every step 0 or +-1 cell along each axis (the hot loop), clipped to [0, M]."""
    ntr = -(-n // track)
    steps = rs.randint(-1, 2, (ntr, track, 2)) * (rs.rand(ntr, track, 2) < 0.6)
    if start is None:
        start = rs.randint(0, M + 1, (ntr, 1, 2))
    pos = np.clip(start + np.cumsum(steps, axis=1), 0, M)
    return pos.reshape(-1, 2)[:n]


def _stream(kind, rs, n, G, K):
    """Footprint origins (x, y) = (u - bias, v - bias), each in [0, G - K]."""
    M = G - K
    if kind == 'slow':
        return _walk(rs, n, M)
    if kind == 'random':
        return rs.randint(0, M + 1, (n, 2))
    if kind == 'one_position':
        return np.tile(rs.randint(0, M + 1, (1, 2)), (n, 1))
    if kind == 'sweep':
        # pure-u and pure-v sweeps, forwards and backwards, from every window origin mod 32,
        # each crossing the window slack several times (column-only / row-only flushes)
        L = min(80, 8 * _slack(K) + 8)
        ramp = np.arange(L + 1)
        out = []
        for o in range(WIN):
            a0 = 8 + o
            b = rs.randint(0, M + 1)
            assert a0 + L <= M
            for axis in (0, 1):
                for a in (a0 + ramp, a0 + L - ramp):
                    p = np.empty((len(a), 2), np.int64)
                    p[:, axis] = a
                    p[:, 1 - axis] = b
                    out.append(p)
        return np.concatenate(out)
    if kind == 'moves':
        # single moves of exactly slack, slack + 1, 31, 32 and 33 cells along u, v and both,
        # each way, three records at each position (the moves fall on every offset in a group)
        c = M // 2
        assert c + 33 <= M and c - 33 >= 0
        out = []
        s = _slack(K)
        for d in (s, s + 1, 31, 32, 33):
            for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1)):
                out += [(c, c)] * 3 + [(c + d * dx, c + d * dy)] * 3
        return np.array(out, np.int64)
    if kind == 'jumps':
        out = []
        base = _walk(rs, 8 * 40, M, track=8 * 40)
        for g in range(40):                     # a jump inside each group of 8, at every offset
            grp = base[8 * g:8 * g + 8].copy()
            grp[g % 8] = rs.randint(0, M + 1, 2)
            out.append(grp)
        for g in range(40):                     # a jump at the start of every group
            out.append(_walk(rs, 8, M, track=8))
        out.append(np.tile(rs.randint(0, M + 1, (1, 2)), (64, 1)))     # 64 at one position
        return np.concatenate(out)
    if kind == 'edges':
        # footprints touching each edge and each corner, sliding along the edge
        out = []
        for fx, fy in ((0, 0), (0, 1), (1, 0), (1, 1), (0, .5), (.5, 0), (1, .5), (.5, 1)):
            x, y = int(fx * M), int(fy * M)
            for t in range(24):
                dx = 0 if fx in (0, 1) else t % 3 - 1
                dy = 0 if fy in (0, 1) else t % 3 - 1
                out.append((np.clip(x + dx, 0, M), np.clip(y + dy, 0, M)))
        return np.array(out, np.int64)
    raise ValueError(kind)


class Case:
    def __init__(self, name, K, OV, W, P, stream, n=0, G=None, seed=None):
        self.name, self.K, self.OV, self.W, self.P, self.stream, self.n = name, K, OV, W, P, stream, n
        self.G = G if G is not None else 2 * ((K + 140 + 1) // 2)
        self.seed = seed if seed is not None else zlib.crc32(name.encode()) & 0xffff
        assert (OV * K) % 2 == 0

    def __repr__(self):
        return self.name


def _inputs(case, degrid=False):
    rs = np.random.RandomState(case.seed + (1 << 20) * degrid)
    K, OV, W, P, G = case.K, case.OV, case.W, case.P, case.G
    xy = _stream(case.stream, rs, case.n, G, K).astype(np.int64)
    n = len(xy)
    bias = (K - 1) // 2 - G // 2
    assert xy.min() >= 0 and xy.max() <= G - K
    sub = rs.randint(0, OV, (n, 2))
    sub[0::5, 0] = 0
    sub[1::5, 0] = OV - 1
    sub[2::5, 1] = 0
    sub[3::5, 1] = OV - 1
    w_plane = rs.randint(0, W, n)
    w_plane[0::6] = 0
    w_plane[1::6] = W - 1
    uv = np.concatenate([xy + bias, sub], axis=1).astype(np.int16)
    return dict(kern=_table(rs, W, OV, K), uv=uv, w_plane=w_plane.astype(np.int16),
                vis=_cint(rs, (n, P), 20 if degrid else 3),
                wg=_density(rs, P, G), weights=rs.randint(1, 4, (n, P)).astype(np.float32),
                grid=_cint(rs, (P, G, G), 4))


def _density(rs, P, G):
    """Density weights in {1, 2, 3}, random, but never equal in neighbouring cells along u (a
    weight read from the wrong cell always shows)."""
    steps = rs.randint(1, 3, (P, G, G))
    return (1 + np.cumsum(steps, axis=2) % 3).astype(np.float32)


def _table(rs, W, OV, K):
    def part():
        return rs.randint(1, 8, (W, OV, K)) * rs.choice([-1, 1], (W, OV, K))
    return (part() + 1j * part()).astype(np.complex64)


def _cint(rs, shape, m):
    return (rs.randint(-m, m + 1, shape) + 1j * rs.randint(-m, m + 1, shape)).astype(np.complex64)


def _l1(z):
    return np.abs(z.real) + np.abs(z.imag)


# ---------------------------------------------------------------------------------------------
# float64 truth (numpy, independent of the oracle), with the simulated bugs of the self-check

MUTATIONS = ('drop_first_u', 'drop_last_u', 'drop_first_v', 'drop_last_v', 'shift', 'sub_row',
             'swap_uv', 'no_conj', 'lose_last', 'wg_neighbour')


def grid_truth(kern, uv, w_plane, vis, wg, mutation=None):
    """grid[p][v0 + j][u0 + k] += vis[p] * wg[p][v + G/2][u + G/2] * conj(kv[j] * ku[k]), the sum
    accumulated with np.bincount per row tap, on a canvas with a one-cell margin (so that a
    shifted footprint stays on it).  Returns (canvas [P][G+2][G+2], bound [P][G+2][G+2]): bound is
    the per-cell sum of |Re| + |Im| products of the factors."""
    kern = np.asarray(kern, np.complex128)
    P, G = wg.shape[0], wg.shape[-1]
    K = kern.shape[-1]
    OV = kern.shape[1]
    uv = uv.astype(np.int64)
    w_plane = w_plane.astype(np.int64)
    vis = np.asarray(vis, np.complex128)
    if mutation == 'lose_last':
        uv, w_plane, vis = uv[:-1], w_plane[:-1], vis[:-1]
    half = G // 2
    bias = (K - 1) // 2 - half
    u, v, su, sv = uv[:, 0], uv[:, 1], uv[:, 2], uv[:, 3]
    x = u - bias + 1 + (mutation == 'shift')
    y = v - bias + 1
    if mutation == 'sub_row':
        sv = (sv + 1) % OV
    kv = kern[w_plane, sv]
    ku = kern[w_plane, su]
    if mutation == 'swap_uv':
        kv, ku = ku, kv
    if mutation != 'no_conj':
        kv, ku = np.conj(kv), np.conj(ku)
    kv, ku = kv.copy(), ku.copy()
    for name, arr, t in (('drop_first_u', ku, 0), ('drop_last_u', ku, K - 1),
                         ('drop_first_v', kv, 0), ('drop_last_v', kv, K - 1)):
        if mutation == name:
            arr[:, t] = 0
    wu = u + half + (mutation == 'wg_neighbour')
    wu = np.where(wu >= G, wu - 2, wu)
    C = G + 2
    out = np.zeros((P, C * C), np.complex128)
    bound = np.zeros((P, C * C))
    taps = np.arange(K)
    cols = x[:, None] + taps[None, :]
    for p in range(P):
        smp = vis[:, p] * wg[p][v + half, wu].astype(np.float64)
        a = smp[:, None] * ku                                   # [N][K] along u
        ab = _l1(smp)[:, None] * _l1(ku)
        for j in range(K):
            idx = ((y + j) * C)[:, None] + cols
            val = a * kv[:, j:j + 1]
            out[p] += np.bincount(idx.ravel(), val.real.ravel(), C * C)
            out[p] += 1j * np.bincount(idx.ravel(), val.imag.ravel(), C * C)
            bound[p] += np.bincount(idx.ravel(), (ab * _l1(kv[:, j:j + 1])).ravel(), C * C)
    return out.reshape(P, C, C), bound.reshape(P, C, C)


def _crop(canvas):
    return canvas[:, 1:-1, 1:-1]


def degrid_truth(kern, uv, w_plane, weights, vis0, grid, mutation=None):
    """vis0 - w * sum_{j,k} kv[j] ku[k] grid[p][v0 + j][u0 + k] (include/kimg.h), and the per
    visibility bound: |w| * sum of |Re| + |Im| products + |vis0|."""
    kern = np.asarray(kern, np.complex128)
    P, G = grid.shape[0], grid.shape[-1]
    K = kern.shape[-1]
    uv = uv.astype(np.int64)
    w_plane = w_plane.astype(np.int64)
    bias = (K - 1) // 2 - G // 2
    x = uv[:, 0] - bias + (mutation == 'shift')
    y = uv[:, 1] - bias
    kv = kern[w_plane, uv[:, 3]].copy()
    ku = kern[w_plane, uv[:, 2]].copy()
    if mutation == 'drop_last_u':
        ku[:, K - 1] = 0
    if mutation == 'drop_last_v':
        kv[:, K - 1] = 0
    g = np.asarray(grid, np.complex128)
    if mutation == 'shift':
        g = np.concatenate([g, np.zeros((P, G, 1))], axis=2)
    n = len(uv)
    s = np.zeros((n, P), np.complex128)
    b = np.zeros((n, P))
    cols = x[:, None] + np.arange(K)[None, :]
    for j in range(K):
        rows = (y + j)[:, None]
        for p in range(P):
            gg = g[p][rows, cols]                               # [N][K]
            s[:, p] += kv[:, j] * np.sum(ku * gg, axis=1)
            b[:, p] += _l1(kv[:, j]) * np.sum(_l1(ku) * _l1(gg), axis=1)
    w = weights.astype(np.float64)
    if mutation == 'no_weight':
        w = np.ones_like(w)
    return np.asarray(vis0, np.complex128) - w * s, w * b + _l1(np.asarray(vis0, np.complex128))


# ---------------------------------------------------------------------------------------------
# cases

# (name, K, OV, W, P, stream, n): W * OV sets where the table lives (see _grid_placement)
GRID_CASES = [
    Case('k1_ov2', 1, 2, 3, 1, 'slow', 3000),
    Case('k2_p2_jumps', 2, 4, 2, 2, 'jumps'),
    Case('k7_edges', 7, 4, 5, 1, 'edges'),
    Case('k8_ov5_p3', 8, 5, 4, 3, 'slow', 2500),
    Case('k8_one_position', 8, 4, 2, 1, 'one_position', 2000),
    Case('k16_ov16_p4_moves', 16, 16, 4, 4, 'moves'),
    Case('k27_sweep', 27, 2, 8, 1, 'sweep'),
    Case('k28_sweep', 28, 8, 4, 1, 'sweep'),
    Case('k28_doubled_rows_8_waves', 28, 8, 35, 1, 'slow', 2000),
    Case('k28_single_rows', 28, 8, 48, 1, 'slow', 3001),
    Case('k28_hbm', 28, 8, 96, 1, 'slow', 3000),
    Case('k28_hbm_p2_jumps', 28, 8, 96, 2, 'jumps'),
    Case('k28_single_rows_p3_moves', 28, 8, 48, 3, 'moves'),
    Case('k31_ov16_p2_moves', 31, 16, 2, 2, 'moves'),
    Case('k32_sweep', 32, 8, 4, 1, 'sweep'),
    Case('k32_edges_p2', 32, 4, 4, 2, 'edges'),
    Case('k33_moves', 33, 8, 4, 1, 'moves'),
    Case('k33_sweep', 33, 8, 4, 1, 'sweep'),
    Case('k45_p3', 45, 2, 6, 3, 'slow', 1200),
    Case('k45_single_rows_edges', 45, 8, 48, 1, 'edges'),
    Case('k60_sweep', 60, 8, 4, 1, 'sweep'),
    Case('k60_hbm', 60, 8, 96, 1, 'slow', 1500),
    Case('k60_p2_jumps', 60, 8, 4, 2, 'jumps'),
    Case('k64_edges', 64, 2, 4, 1, 'edges'),
    Case('k64_p4_moves', 64, 4, 2, 4, 'moves'),
    Case('k65_generic', 65, 2, 2, 1, 'slow', 400),
    Case('k96_generic_p2', 96, 4, 2, 2, 'edges'),
] + [Case('count_%d' % n, 8, 4, 4, 1 + (n % 2), 'slow', n)
     for n in (1, 2, 3, 7, 8, 9, 63, 64, 65, 127, 128, 129, 1001, 3003)]

DEGRID_CASES = [
    Case('dk1', 1, 2, 3, 1, 'slow', 3000),
    Case('dk2_jumps', 2, 4, 2, 2, 'jumps'),
    Case('dk7_edges', 7, 4, 5, 1, 'edges'),
    Case('dk8_ov5_p3_random', 8, 5, 4, 3, 'random', 2500),
    Case('dk16_ov16_p4_moves', 16, 16, 4, 4, 'moves'),
    Case('dk27_sweep', 27, 2, 8, 1, 'sweep'),
    Case('dk28_random', 28, 8, 4, 1, 'random', 2000),
    Case('dk28_single_rows', 28, 8, 48, 1, 'slow', 3001),
    Case('dk28_hbm_p2', 28, 8, 96, 2, 'random', 1500),
    Case('dk31_moves', 31, 16, 2, 2, 'moves'),
    Case('dk32_edges', 32, 8, 4, 1, 'edges'),
    Case('dk33_sweep', 33, 8, 4, 1, 'sweep'),
    Case('dk45_hbm_pair_lds_diag', 45, 8, 48, 3, 'random', 800),
    Case('dk60_hbm', 60, 8, 96, 1, 'slow', 1000),
    Case('dk60_p2_random', 60, 4, 4, 2, 'random', 700),
    Case('dk64_edges', 64, 2, 4, 1, 'edges'),
    Case('dk65_generic', 65, 2, 2, 1, 'random', 300),
    Case('dk96_generic', 96, 4, 2, 2, 'edges'),
] + [Case('dcount_%d' % n, 8, 4, 4, 1 + (n % 2), 'random', n)
     for n in (1, 2, 3, 15, 16, 17, 63, 64, 65, 1001)]

LONG = Case('long_launch', 2, 4, 64, 1, 'slow', 8 << 20, G=2048, seed=11)
SCATTERED = Case('scattered', 8, 4, 4, 2, 'random', 65536 + 37, G=512, seed=12)


def _grid_case_uncached(case):
    inp = _inputs(case)
    canvas, bound = grid_truth(inp['kern'], inp['uv'], inp['w_plane'], inp['vis'], inp['wg'])
    return inp, _crop(canvas), _crop(bound)


# (LONG, hundreds of MB, is never cached: its tests build it on their own)
_grid_case = functools.lru_cache(maxsize=None)(_grid_case_uncached)


@functools.lru_cache(maxsize=None)
def _degrid_case(case):
    inp = _inputs(case, degrid=True)
    want, bound = degrid_truth(inp['kern'], inp['uv'], inp['w_plane'], inp['weights'], inp['vis'],
                               inp['grid'])
    return inp, want, bound


def _grid_fits_lds(P, W, OV, K):
    """tables_fit_lds of grid_mfma.hip (LDS budget 160 KiB; staging per wave 64 * (16 + 16 P)
    bytes, P counted as 2 when there are more)."""
    return _grid_lds(1 if P == 1 else 2, W, OV, 8, 32, 2 if K > WIN else 1) <= 160 * 1024


def _grid_lds(pn, W, OV, nw, row, tables=1):
    return tables * W * OV * row * 8 + nw * 64 * (16 + 16 * pn)


def _grid_placement(P, W, OV, K):
    """Where the gridder's window kernel reads its table in each launch over polarizations (P = 3
    runs as 2 + 1, P = 4 as 2 + 2), restating table_in_lds and the launch choice of
    kimg_grid_mfma: doubled rows when they fit the LDS (8 waves or more), single rows, or a padded
    copy in HBM; widths above 32 add off-diagonal tap blocks, always read from HBM."""
    limit = 160 * 1024
    out = []
    for pn in [2] * (P // 2) + [1] * (P % 2):
        # narrow kernels: table_in_lds for the whole call; the diagonal blocks of wide ones: the
        # one-table budget of this launch
        in_lds = _grid_fits_lds(P, W, OV, K) if K <= WIN else _grid_lds(pn, W, OV, 8, 32) <= limit
        where = 'hbm' if not in_lds else \
            ('lds_doubled' if _grid_lds(pn, W, OV, 8, 64) <= limit else 'lds_single')
        out.append(where + ('+offdiag_hbm' if K > WIN else ''))
    return tuple(out)


def _degrid_placement(W, OV, K):
    """The same for the degridder (degrid_mfma.hip: 12-wave budget, rows of taps + 1)."""
    def lds(taps, tables=1):
        return tables * W * OV * (taps + 1) * 8 + 12 * 64 * 16
    limit = 160 * 1024
    if lds(32, 2 if K > WIN else 1) > limit:
        diag = 'lds_single' if lds(32) <= limit else 'hbm'
        return diag + '+offdiag_hbm' if K > WIN else 'hbm'
    return 'lds_doubled' if lds(64) <= limit else 'lds_single'


# ---------------------------------------------------------------------------------------------
# CPU: the harness checks itself

def test_matrix_covers_the_issue():
    """Widths, oversampling, polarizations and table placements the matrix must contain."""
    ks = {c.K for c in GRID_CASES}
    assert {1, 2, 7, 8, 16, 27, 28, 31, 32, 33, 45, 60, 64, 65, 96} <= ks
    assert {1, 2, 7, 8, 16, 27, 28, 31, 32, 33, 45, 60, 64, 65, 96} <= {c.K for c in DEGRID_CASES}
    assert {2, 4, 8, 16} <= {c.OV for c in GRID_CASES} and any(c.OV % 2 for c in GRID_CASES)
    assert {1, 2, 3, 4} <= {c.P for c in GRID_CASES} and {1, 2, 3, 4} <= {c.P for c in DEGRID_CASES}
    gp = {w for c in GRID_CASES if c.K <= 2 * WIN for w in _grid_placement(c.P, c.W, c.OV, c.K)}
    assert {'lds_doubled', 'lds_single', 'hbm', 'lds_doubled+offdiag_hbm',
            'lds_single+offdiag_hbm', 'hbm+offdiag_hbm'} <= gp
    dp = {_degrid_placement(c.W, c.OV, c.K) for c in DEGRID_CASES if c.K <= 2 * WIN}
    assert {'lds_doubled', 'lds_single', 'hbm', 'lds_single+offdiag_hbm', 'hbm+offdiag_hbm'} <= dp


def _self_check_cases():
    return [c for c in GRID_CASES if len(_stream(c.stream, np.random.RandomState(0), c.n, c.G, c.K))
            * c.K * c.K * c.P <= 4_000_000]


@pytest.mark.parametrize('case', _self_check_cases(), ids=repr)
def test_truth_sees_every_simulated_bug(case):
    """On the harness's own inputs the float64 truth moves at least one cell under each simulated
    bug (with K = 1 a u / v swap is no bug: kv[0] ku[0] = ku[0] kv[0])."""
    inp = _inputs(case)
    args = (inp['kern'], inp['uv'], inp['w_plane'], inp['vis'], inp['wg'])
    want, _ = grid_truth(*args)
    assert np.all(want.real == np.round(want.real)) and np.count_nonzero(want)
    for m in MUTATIONS:
        if m == 'swap_uv' and case.K == 1:
            continue
        got, _ = grid_truth(*args, mutation=m)
        assert not np.array_equal(got, want), m


@pytest.mark.parametrize('case', DEGRID_CASES[:12], ids=repr)
def test_degrid_truth_sees_simulated_bugs(case):
    inp = _inputs(case, degrid=True)
    args = (inp['kern'], inp['uv'], inp['w_plane'], inp['weights'], inp['vis'], inp['grid'])
    want, _ = degrid_truth(*args)
    for m in ('drop_last_u', 'drop_last_v', 'shift', 'no_weight'):
        got, _ = degrid_truth(*args, mutation=m)
        assert not np.array_equal(got, want), m


@pytest.mark.parametrize('case', GRID_CASES + [SCATTERED], ids=repr)
def test_premise_gridder(case):
    """Every partial sum of every GPU gridder case stays below 2^24 (prefill and padding cases
    reuse these inputs with |prefill| <= 100)."""
    _, want, bound = _grid_case(case)
    assert bound.max() + 200 < EXACT
    assert np.count_nonzero(want)


@pytest.mark.parametrize('case', DEGRID_CASES + [SCATTERED], ids=repr)
def test_premise_degridder(case):
    _, _, bound = _degrid_case(case)
    assert bound.max() < EXACT


def test_premise_long_launch_and_production_order():
    _, _, bound = _grid_case_uncached(LONG)
    assert bound.max() < EXACT
    inp = _inputs(LONG, degrid=True)
    _, bound = degrid_truth(inp['kern'], inp['uv'], inp['w_plane'], inp['weights'], inp['vis'],
                            inp['grid'])
    assert bound.max() < EXACT
    for K, OV, W, P in PRODUCTION:
        arrival = _arrival(K, OV, W, P)
        _, bound = grid_truth(arrival['kern'], arrival['uv'], arrival['w_plane'], arrival['vis'],
                              arrival['wg'])
        assert bound.max() < EXACT
        _, bound = degrid_truth(arrival['kern'], arrival['uv'], arrival['w_plane'],
                                arrival['weights'], arrival['vis'], arrival['grid'])
        assert bound.max() < EXACT


def _split_f16(x):
    """split_f16 / split_tap / row_operand of grid_mfma.hip on float32 values: hi = fp16(x) rounded
    to nearest, lo = fp16(x - hi)."""
    x = np.asarray(x, np.float32)
    with np.errstate(over='ignore'):
        hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def _split_is_exact(x):
    hi, lo = _split_f16(x)
    return bool(np.all(np.isfinite(hi)) and np.array_equal(
        hi.astype(np.float64) + lo.astype(np.float64), np.asarray(x, np.float64)))


def test_split_fp16_keeps_11_bit_integers():
    """The fp16 form is exact for operands of up to 11 bits (module docstring): at every table
    scale S = 2^(13 - e_k) and sample scale T = 2^-E (e_k, E = 0..10), every tap times S splits
    into hi = tap, lo = 0, and every row operand r S T (r an integer up to
    2 (2^(e_k+1) - 1)(2^(E+1) - 1), the largest |Re s conj kv|) splits into hi + lo exactly and
    finitely -- exhaustively at the largest scales, at the end points and at random elsewhere.  A
    12-bit operand does round.  The harness's inputs stay far inside 11 bits."""
    rs = np.random.RandomState(3)
    big = 2 * 2047 * 2047
    assert big < (1 << 23)
    # e_k = E = 10: every integer 0 .. big at scale S T = 2^3 2^-10
    assert _split_is_exact(np.arange(big + 1, dtype=np.float32) * np.float32(2.0 ** -7))
    for e_k in range(11):
        S = 2.0 ** (13 - e_k)
        taps = np.arange(1, 1 << (e_k + 1), dtype=np.float32) * np.float32(S)
        hi, lo = _split_f16(taps)
        assert np.array_equal(hi.astype(np.float32), taps) and not np.any(lo)
        for E in range(11):
            top = 2 * ((1 << (e_k + 1)) - 1) * ((1 << (E + 1)) - 1)
            r = np.concatenate([np.arange(0, min(top, 4096) + 1), np.arange(max(top - 4096, 0), top + 1),
                                rs.randint(0, top + 1, 20000)]).astype(np.float32)
            assert _split_is_exact(r * np.float32(S * 2.0 ** -E)), (e_k, E)
            assert S * 2.0 ** -E >= 2.0 ** -22
    # one bit more and the pair no longer holds every operand
    assert not _split_is_exact(np.arange(1 << 23, 1 << 24, dtype=np.float32) * np.float32(2.0 ** -10))
    # the harness: taps and samples of at most 4 bits, grid values of at most 3
    for case in GRID_CASES[:8]:
        inp = _inputs(case)
        assert np.abs(inp['kern'].view(np.float32)).max() < 8
        assert np.abs(inp['vis'].view(np.float32)).max() * inp['wg'].max() < 16
        assert np.abs(_inputs(case, degrid=True)['grid'].view(np.float32)).max() < 8


# ---------------------------------------------------------------------------------------------
# GPU harness

def _lib():
    from katsdpimager_amd._lib import lib
    return lib()


def _dev(ctx, q, a):
    from katsdpimager_amd import accel
    a = np.ascontiguousarray(a)
    d = accel.DeviceArray(ctx, a.shape, a.dtype)
    d.set(q, a)
    return d


def _workspace(ctx, nbytes):
    from katsdpimager_amd import accel
    if nbytes == 0:
        return None, 0
    return accel.DeviceArray(ctx, (int(nbytes),), np.uint8), int(nbytes)


def run_grid(ctx, q, case, inp, variant, arith, prefill=None, rpad=0, vpad=0, wg_pad=(0, 0),
             workspace=True):
    from katsdpimager_amd import grid
    from katsdpimager_amd._lib import check
    L = _lib()
    P, G, K, W, OV = case.P, case.G, case.K, case.W, case.OV
    n = len(inp['uv'])
    g0 = np.zeros((P, G, G), np.complex64) if prefill is None else prefill
    g = Padded(ctx, q, g0, rpad, vpad, np.complex64(-1.5e7 + 3.25e6j))
    wg = Padded(ctx, q, inp['wg'], wg_pad[0], wg_pad[1], np.float32(1e6))
    table = _dev(ctx, q, inp['kern'])
    uv, wp, vis = _dev(ctx, q, inp['uv']), _dev(ctx, q, inp['w_plane']), _dev(ctx, q, inp['vis'])
    if variant == 'binned':
        nbytes = L.kimg_grid_binned_workspace_bytes(n, P, W, OV, K)
    else:
        nbytes = L.kimg_grid_workspace_bytes(n, P, W, OV, K)
    ws, nbytes = _workspace(ctx, nbytes) if workspace else (None, 0)
    rc = L.kimg_grid(g.dev.ptr, g.row, g.pol, G, P, wg.dev.ptr, wg.row, wg.pol, uv.ptr, wp.ptr,
                     vis.ptr, n, table.ptr, W, OV, K, ws.ptr if ws is not None else None, nbytes,
                     grid.GRID_VARIANTS[variant], grid.GRID_ARITH[arith], q.handle)
    check(rc, 'kimg_grid %s %s' % (variant, arith))
    q.finish()
    wg.get(q)
    return g.get(q)


def run_degrid(ctx, q, case, inp, variant, arith, rpad=0, vpad=0):
    from katsdpimager_amd import grid
    from katsdpimager_amd._lib import check
    L = _lib()
    P, G, K, W, OV = case.P, case.G, case.K, case.W, case.OV
    n = len(inp['uv'])
    g = Padded(ctx, q, inp['grid'], rpad, vpad, np.complex64(3e6 - 5e6j))
    table = _dev(ctx, q, inp['kern'])
    uv, wp = _dev(ctx, q, inp['uv']), _dev(ctx, q, inp['w_plane'])
    weights, vis = _dev(ctx, q, inp['weights']), _dev(ctx, q, inp['vis'])
    if variant == 'binned':
        nbytes = L.kimg_degrid_binned_workspace_bytes(n, P, W, OV, K)
    else:
        nbytes = L.kimg_degrid_workspace_bytes(P, W, OV, K)
    ws, nbytes = _workspace(ctx, nbytes)
    rc = L.kimg_degrid(g.dev.ptr, g.row, g.pol, G, P, uv.ptr, wp.ptr, weights.ptr, vis.ptr, n,
                       table.ptr, W, OV, K, ws.ptr if ws is not None else None, nbytes,
                       grid.GRID_VARIANTS[variant], grid.GRID_ARITH[arith], q.handle)
    check(rc, 'kimg_degrid %s %s' % (variant, arith))
    q.finish()
    g.get(q)
    return vis.get(q)


def _assert_exact(got, want, what):
    bad = got.astype(np.complex128) != want
    assert not bad.any(), '%s: %d cells differ, first at %s: got %s, want %s' % (
        what, int(bad.sum()), np.argwhere(bad)[0], got[tuple(np.argwhere(bad)[0])],
        want[tuple(np.argwhere(bad)[0])])


def _bits(a):
    return (a + np.complex64(0)).view(np.uint32)        # (-0 + 0 = +0: only values compared)


def _assert_grid_placement(case):
    L = _lib()
    P, W, OV, K = case.P, case.W, case.OV, case.K
    nbytes = L.kimg_grid_workspace_bytes(1, P, W, OV, K)
    where = _grid_placement(P, W, OV, K)
    if K > 2 * WIN:
        assert nbytes == 0
    elif K <= WIN and all(w.startswith('lds_') for w in where):
        assert nbytes == 256
    else:
        # a padded copy in HBM: one table of [W OV][64] rows, two for the off-diagonal blocks
        # (widths above 32 always have them, wherever their diagonal blocks read from)
        assert nbytes == W * OV * 64 * 8 * (2 if K > WIN else 1) + 256
    return where


@pytest.mark.gpu
@pytest.mark.parametrize('case', GRID_CASES, ids=repr)
def test_grid_exact(case):
    """Every variant and arithmetic form against the float64 truth, bit for bit, and against one
    another.  K > 64: `auto` routes to the generic kernel, `mfma` and `binned` are unsupported."""
    ctx, q = context_queue()
    inp, want, bound = _grid_case(case)
    assert bound.max() < EXACT
    _assert_grid_placement(case)
    runs = [('generic', 'fp32')]
    if case.K <= 2 * WIN:
        runs += [(v, a) for v in ('mfma', 'binned', 'auto') for a in GRID_FORMS]
    else:
        runs += [('auto', a) for a in GRID_FORMS]
    got = {}
    for variant, arith in runs:
        got[variant, arith] = run_grid(ctx, q, case, inp, variant, arith)
        _assert_exact(got[variant, arith], want, '%s/%s' % (variant, arith))
    first = _bits(got[runs[0]])
    for key, g in got.items():
        assert np.array_equal(_bits(g), first), key
    if case.K > 2 * WIN:
        from katsdpimager_amd._lib import KimgError
        for variant in ('mfma', 'binned'):
            with pytest.raises(KimgError) as e:
                run_grid(ctx, q, case, inp, variant, 'fp32')
            assert e.value.code == KIMG_EUNSUPPORTED


EDGE_CASES = [c for c in GRID_CASES if c.name in ('k28_single_rows_p3_moves', 'k45_p3', 'k7_edges',
                                                  'k60_hbm', 'k16_ov16_p4_moves')]


@pytest.mark.gpu
@pytest.mark.parametrize('case', EDGE_CASES, ids=repr)
def test_grid_adds_to_prefill_with_padded_strides(case):
    """A pre-filled grid comes out as prefill + truth (the gridder adds, never overwrites), with
    padded row and polarization strides of the grid and of the density weights; the padding
    (sentinels) is bit-identical afterwards."""
    ctx, q = context_queue()
    inp, want, bound = _grid_case(case)
    rs = np.random.RandomState(5)
    prefill = _cint(rs, want.shape, 100)
    assert bound.max() + 200 < EXACT
    for variant in ('generic', 'mfma', 'binned', 'auto'):
        for arith in (GRID_FORMS if variant != 'generic' else ('fp32',)):
            got = run_grid(ctx, q, case, inp, variant, arith, prefill=prefill, rpad=7, vpad=3,
                           wg_pad=(5, 2))
            _assert_exact(got, want + prefill, 'prefill/padded %s/%s' % (variant, arith))


@pytest.mark.gpu
def test_grid_long_launch_by_the_chunk():
    """One launch long enough for the window kernel to hand out its work by the chunk (at least
    2 x 1024 visibilities per wave), with the chunk counter in the workspace and without a
    workspace (table in LDS: chunks taken in a fixed order); fp32 pair form and fp16 form."""
    ctx, q = context_queue()
    case = LONG
    inp, want, bound = _grid_case_uncached(case)
    assert bound.max() < EXACT
    assert _assert_grid_placement(case) == ('lds_doubled',)
    # 12-wave blocks, one per CU: the doubled table (256 rows) takes more than half the LDS
    # (launch() of grid_mfma.hip)
    assert 2 * (case.W * case.OV * 64 * 8 + 12 * 64 * 32) > 160 * 1024
    waves = 12 * _lib().kimg_get_window_cus()
    assert waves > 0 and len(inp['uv']) >= 2 * 1024 * waves
    for arith, ws in (('fp32', True), ('fp32', False), ('split_fp16', True)):
        got = run_grid(ctx, q, case, inp, 'mfma', arith, workspace=ws)
        _assert_exact(got, want, 'long %s workspace=%s' % (arith, ws))


@pytest.mark.gpu
def test_grid_scattered_binned():
    """65 573 visibilities at random cells (no locality) through the binned variant, every form,
    and the direct window kernel for comparison."""
    ctx, q = context_queue()
    inp, want, bound = _grid_case(SCATTERED)
    assert bound.max() < EXACT
    for variant, arith in [('binned', a) for a in GRID_FORMS] + [('mfma', 'fp32')]:
        got = run_grid(ctx, q, SCATTERED, inp, variant, arith)
        _assert_exact(got, want, 'scattered %s/%s' % (variant, arith))


@pytest.mark.gpu
@pytest.mark.parametrize('case', DEGRID_CASES, ids=repr)
def test_degrid_exact(case):
    """generic, mfma and binned in both forms: vis0 - w * sum, bit for bit.  K > 64: `auto` routes
    to the generic kernel."""
    ctx, q = context_queue()
    inp, want, bound = _degrid_case(case)
    assert bound.max() < EXACT
    L = _lib()
    nbytes = L.kimg_degrid_workspace_bytes(case.P, case.W, case.OV, case.K)
    where = _degrid_placement(case.W, case.OV, case.K)
    if case.K > 2 * WIN:
        assert nbytes == 0
        runs = [('generic', 'fp32'), ('auto', 'fp32'), ('auto', 'split_fp16')]
    else:
        # 256 bytes: every table in LDS; else a padded copy of [W OV][65] rows (two for K > 32)
        in_lds = where in ('lds_doubled', 'lds_single')
        assert nbytes == (256 if in_lds else
                          case.W * case.OV * 65 * 8 * (2 if case.K > WIN else 1) + 256)
        runs = [('generic', 'fp32')] + [(v, a) for v in ('mfma', 'binned') for a in DEGRID_FORMS]
    for variant, arith in runs:
        got = run_degrid(ctx, q, case, inp, variant, arith)
        _assert_exact(got, want, '%s/%s' % (variant, arith))


DEGRID_PAD_CASES = [c for c in DEGRID_CASES if c.name in ('dk28_random', 'dk45_hbm_pair_lds_diag',
                                                          'dk7_edges')]


@pytest.mark.gpu
@pytest.mark.parametrize('case', DEGRID_PAD_CASES, ids=repr)
def test_degrid_padded_strides(case):
    """Padded grid strides with large values in the padding: any sum that read them would be off
    by millions."""
    ctx, q = context_queue()
    inp, want, bound = _degrid_case(case)
    assert bound.max() < EXACT
    for variant in ('generic', 'mfma', 'binned'):
        for arith in (DEGRID_FORMS if variant != 'generic' else ('fp32',)):
            got = run_degrid(ctx, q, case, inp, variant, arith, rpad=9, vpad=4)
            _assert_exact(got, want, 'padded %s/%s' % (variant, arith))


@pytest.mark.gpu
def test_degrid_scattered_and_long():
    """65 573 scattered visibilities through binned (both forms), and a long launch by the chunk."""
    ctx, q = context_queue()
    inp, want, bound = _degrid_case(SCATTERED)
    assert bound.max() < EXACT
    for variant, arith in (('binned', 'fp32'), ('binned', 'split_fp16'), ('mfma', 'fp32')):
        _assert_exact(run_degrid(ctx, q, SCATTERED, inp, variant, arith), want,
                      'scattered %s/%s' % (variant, arith))
    inp = _inputs(LONG, degrid=True)
    want, bound = degrid_truth(inp['kern'], inp['uv'], inp['w_plane'], inp['weights'], inp['vis'],
                               inp['grid'])
    assert bound.max() < EXACT
    for arith in DEGRID_FORMS:
        _assert_exact(run_degrid(ctx, q, LONG, inp, 'mfma', arith), want, 'long %s' % arith)


# ---------------------------------------------------------------------------------------------
# production order: arrival stream -> kimg_store_reorder -> window kernels

PRODUCTION = [(28, 8, 32, 2), (45, 4, 8, 1)]


@functools.lru_cache(maxsize=None)
def _arrival(K, OV, W, P):
    """Integer counterpart of test_preprocess_gpu._arrival_stream: baseline-sorted blocks of slowly
    moving tracks that come back to the same cells in later blocks, plus scattered records,
    clipped to the footprint contract; w_plane constant over runs of 97 records of the tracks."""
    rs = np.random.RandomState(K * 7 + P)
    G = 2 * ((K + 200) // 2)
    bias = (K - 1) // 2 - G // 2
    M = G - K
    n_track, n_scatter, repeat, tracks = 12000, 2000, 3, 40
    per = n_track // (tracks * repeat)
    start = rs.uniform(0, M, (tracks, 2))
    speed = rs.uniform(-0.2, 0.2, (tracks, 2))
    pieces = []
    for block in range(repeat):
        for t in range(tracks):
            pieces.append(start[t] + speed[t] * (np.arange(per) + 0.25 * per * block)[:, None])
    pos = np.concatenate(pieces + [rs.uniform(0, M, (n_scatter, 2))])
    fine = np.floor(np.clip(pos, 0, M + 0.999) * OV).astype(np.int64)
    n = len(fine)
    uv = np.concatenate([fine // OV + bias, fine % OV], axis=1).astype(np.int16)
    nt = per * tracks * repeat
    w_plane = rs.randint(0, W, n)
    w_plane[:nt] = (np.arange(nt) // 97) % W
    return dict(kern=_table(rs, W, OV, K), uv=uv, w_plane=w_plane.astype(np.int16),
                vis=_cint(rs, (n, P), 3), wg=_density(rs, P, G),
                weights=rs.randint(1, 4, (n, P)).astype(np.float32), grid=_cint(rs, (P, G, G), 4),
                G=G)


@pytest.mark.gpu
@pytest.mark.parametrize('K,OV,W,P', PRODUCTION)
def test_production_order_exact(K, OV, W, P):
    """The arrival stream through kimg_store_reorder (merge off and on; merged runs are float32 sums
    of integers, exact), the stored records gridded with the window kernel: bit for bit the float64
    truth of the arrival stream.  The unmerged store degridded: per record vis0 - w * sum."""
    from katsdpimager_amd import accel
    from katsdpimager_amd._lib import check
    ctx, q = context_queue()
    a = _arrival(K, OV, W, P)
    canvas, bound = grid_truth(a['kern'], a['uv'], a['w_plane'], a['vis'], a['wg'])
    assert bound.max() < EXACT
    want = _crop(canvas)
    n = len(a['uv'])
    L = _lib()
    case = Case('production', K, OV, W, P, 'slow', n, G=a['G'])
    for merge in (0, 1):
        d = [_dev(ctx, q, a[k]) for k in ('uv', 'w_plane', 'weights', 'vis')]
        o = [accel.DeviceArray(ctx, a[k].shape, a[k].dtype) for k in ('uv', 'w_plane', 'weights', 'vis')]
        count = accel.DeviceArray(ctx, (1,), np.int64)
        ws, nbytes = _workspace(ctx, L.kimg_store_reorder_workspace_bytes(n))
        check(L.kimg_store_reorder(P, n, K, OV, W, merge, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr,
                                   o[0].ptr, o[1].ptr, o[2].ptr, o[3].ptr, count.ptr, ws.ptr, nbytes,
                                   q.handle), 'kimg_store_reorder')
        m = int(count.get(q)[0])
        assert (m == n) if not merge else (0 < m < n)
        stored = dict(a, uv=o[0].get(q)[:m], w_plane=o[1].get(q)[:m], weights=o[2].get(q)[:m],
                      vis=o[3].get(q)[:m])
        for arith in GRID_FORMS:
            got = run_grid(ctx, q, case, stored, 'mfma', arith)
            _assert_exact(got, want, 'store merge=%d %s' % (merge, arith))
        if not merge:
            dwant, bound = degrid_truth(a['kern'], stored['uv'], stored['w_plane'],
                                        stored['weights'], stored['vis'], a['grid'])
            assert bound.max() < EXACT
            for arith in DEGRID_FORMS:
                stored_d = dict(stored, grid=a['grid'])
                got = run_degrid(ctx, q, case, stored_d, 'mfma', arith)
                _assert_exact(got, dwant, 'store degrid %s' % arith)
