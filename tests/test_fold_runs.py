"""The window gridder folds runs of consecutive records with equal (u, v, sub_u, sub_v, w_plane)
into one update (grid_mfma.hip, "fold runs"; include/kimg.h, KIMG_ARITH_NO_FOLD).

* exact: integer-valued inputs whose every partial sum stays below 2^24 (the premise of
  test_exact_gridding.py, asserted per case), streams built from runs of 1, 2, 3, 8, 63, 64, 65 and
  200 equal records that straddle the kernel's batches of 64 and -- in the long case, which is cut
  into chunks -- its chunks, a run whose samples cancel, runs interrupted by a record that fails
  the range checks: fold on, fold off, the oracle and a float64 truth agree bit for bit.
* no duplicates: on a stream that was merged before, fold on and fold off run the same
  instructions; the grids differ by the order of the float atomics only.
* rounded: on a duplicate-heavy float stream the folded grid is as close to a float64 truth as
  the unfolded one.

The CPU tests check the streams themselves and the tuning key."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from helpers import context_queue        # noqa: E402
from test_exact_gridding import (EXACT, Padded, _assert_exact, _bits, _cint, _crop,     # noqa: E402
                                 _density, _dev, _table, _workspace, grid_truth)

NO_FOLD = 0x100                         # KIMG_ARITH_NO_FOLD
RUN_LENGTHS = (1, 2, 3, 8, 63, 64, 65, 200)
FORMS = ('fp32', 'fp32_32x32', 'split_fp16')


class FoldCase:
    def __init__(self, name, K, OV, W, P, n, G, cus=0, amp=2):
        self.name, self.K, self.OV, self.W, self.P, self.n, self.G = name, K, OV, W, P, n, G
        self.cus, self.amp = cus, amp

    def __repr__(self):
        return self.name


# k28_long: gridded on ONE compute unit (KIMG_WINDOW_CUS(1)), where 40 000 records are a long launch:
# the stream is then cut into chunks (multiples of 64) that the waves take from a counter
CASES = [
    FoldCase('k28_p1', 28, 8, 4, 1, 6000, 168),
    FoldCase('k28_p2', 28, 8, 4, 2, 6000, 168),
    FoldCase('k28_p3', 28, 8, 4, 3, 6000, 168),
    FoldCase('k28_hbm_p1', 28, 8, 96, 1, 6000, 168),
    FoldCase('k60_p1', 60, 8, 4, 1, 5000, 200),
    FoldCase('k28_long_chunks', 28, 8, 4, 1, 40000, 256, cus=1, amp=1),
]


def fold_stream(case):
    """Records in runs of equal (u, v, sub_u, sub_v, w_plane).  Returns the inputs of kimg_grid, the
    mask of the records that pass the range checks, and the run lengths (of equal keys, the
    interrupting records counted as runs of their own)."""
    rs = np.random.RandomState(sum(map(ord, case.name)))
    K, OV, W, P, G = case.K, case.OV, case.W, case.P, case.G
    M = G - K
    bias = (K - 1) // 2 - G // 2
    uv, wp, vis, ok = [], [], [], []
    pos = rs.randint(0, M + 1, 2)
    last_key = None
    specials = ['cancel', 'bad_w', 'bad_sub'] * 3
    i = 0
    while sum(len(r) for r in uv) < case.n:
        # the listed lengths first, at shifting phases against the batches of 64, then short runs
        if i < 4 * len(RUN_LENGTHS):
            L = RUN_LENGTHS[i % len(RUN_LENGTHS)]
            if i % len(RUN_LENGTHS) == 0:
                L += (7, 0, 29, 50)[i // len(RUN_LENGTHS)]     # shifts the phase of what follows
        else:
            L = int(rs.choice([1, 1, 2, 3, 4, 5, 7, 9, 12, 17, 40]))
        kind = 'plain'
        if i >= 4 * len(RUN_LENGTHS) and i % 9 == 0 and specials:
            kind = specials.pop()
            L = max(L, 6)
        if i % 37 == 36:
            pos = rs.randint(0, M + 1, 2)                       # a jump
        else:
            pos = np.clip(pos + rs.randint(-1, 2, 2) * (rs.rand(2) < 0.6), 0, M)
        sub = rs.randint(0, OV, 2)
        w = rs.randint(0, W)
        key = (pos[0], pos[1], sub[0], sub[1], w)
        if key == last_key:
            sub[0] = (sub[0] + 1) % OV
            key = (pos[0], pos[1], sub[0], sub[1], w)
        last_key = key
        v = _cint(rs, (L, P), case.amp)
        if kind == 'cancel':
            L -= L % 2
            v = v[:L]
            v[L // 2:] = -v[:L // 2]
        rec = np.tile(np.array([pos[0] + bias, pos[1] + bias, sub[0], sub[1]], np.int64), (L, 1))
        wl = np.full(L, w, np.int64)
        good = np.ones(L, bool)
        if kind == 'bad_w':
            wl[L // 2] = W                                      # same uv words, plane out of range
            good[L // 2] = False
        if kind == 'bad_sub':
            rec[L // 2, 2] = OV                                 # sub_u out of range
            good[L // 2] = False
        uv.append(rec)
        wp.append(wl)
        vis.append(v)
        ok.append(good)
        i += 1
    uv = np.concatenate(uv).astype(np.int16)
    wp = np.concatenate(wp).astype(np.int16)
    vis = np.concatenate(vis)
    ok = np.concatenate(ok)
    return dict(kern=_table(rs, W, OV, K), uv=uv, w_plane=wp, vis=vis, wg=_density(rs, P, G)), ok


def run_lengths(inp):
    key = np.concatenate([inp['uv'].astype(np.int64), inp['w_plane'].astype(np.int64)[:, None]], axis=1)
    head = np.ones(len(key), bool)
    head[1:] = np.any(key[1:] != key[:-1], axis=1)
    starts = np.flatnonzero(head)
    return starts, np.diff(np.append(starts, len(key)))


def _truth(inp, ok):
    canvas, bound = grid_truth(inp['kern'], inp['uv'][ok], inp['w_plane'][ok], inp['vis'][ok], inp['wg'])
    return _crop(canvas), _crop(bound)


@pytest.mark.parametrize('case', CASES, ids=repr)
def test_streams_hold_the_runs_they_claim(case):
    """The listed run lengths occur, runs straddle multiples of 64 (and of every chunk length, which
    is one), a run cancels, runs are interrupted by records that fail the range checks; the
    exactness premise holds."""
    inp, ok = fold_stream(case)
    starts, lengths = run_lengths(inp)
    for L in RUN_LENGTHS[1:]:
        assert np.any(lengths == L), L
    assert np.any(lengths == 1)
    ends = starts + lengths
    straddle = (starts // 64 != (ends - 1) // 64) & (starts % 64 != 0)
    assert straddle.sum() >= 8
    assert np.any(straddle & (lengths >= 63))
    # every phase of a run's start against the batch is not needed; many different ones are
    assert len(set((starts[lengths > 1] % 64).tolist())) >= 32
    assert (~ok).sum() >= 4
    bad = np.flatnonzero(~ok)
    u = inp['uv'].astype(np.int64)
    for b in bad:       # the interrupting record sits inside a run: its neighbours share one key
        assert np.array_equal(u[b - 1], u[b + 1]) and inp['w_plane'][b - 1] == inp['w_plane'][b + 1]
    # a run of two or more whose samples sum to zero
    sums = np.add.reduceat(inp['vis'], starts, axis=0)
    assert np.any((lengths >= 4) & np.all(sums == 0, axis=1))
    _, bound = _truth(inp, ok)
    assert bound.max() < EXACT
    # most records repeat their predecessor: the fold has work to do
    assert len(starts) < 0.3 * len(u)


def test_tuning_key():
    from katsdpimager_amd import grid
    assert grid._tuning(None) == (0, 0, True)
    assert grid._tuning({'fold_runs': False, 'arith': 'split_fp16'}) == (0, 1, False)
    assert grid._tuning({'fold_runs': True}, np.float64) == (0, 0, True)
    with pytest.raises(ValueError):
        grid._tuning({'fold_runs': 'no'})
    with pytest.raises(ValueError):
        grid._tuning({'fold': False})
    assert grid.GRID_ARITH_NO_FOLD == NO_FOLD
    with open(os.path.join(ROOT, 'include', 'kimg.h')) as f:
        assert '#define KIMG_ARITH_NO_FOLD 0x100' in f.read()


# ---------------------------------------------------------------------------------------------
# GPU

def _run(ctx, q, case, inp, variant, arith, fold):
    from katsdpimager_amd import grid
    from katsdpimager_amd._lib import check, lib
    L = lib()
    P, G, K, W, OV = case.P, case.G, case.K, case.W, case.OV
    n = len(inp['uv'])
    g = Padded(ctx, q, np.zeros((P, G, G), np.complex64), 3, 1, np.complex64(-1.5e7 + 3.25e6j))
    wg = Padded(ctx, q, inp['wg'], 0, 0, np.float32(1e6))
    table = _dev(ctx, q, inp['kern'])
    uv, wp, vis = _dev(ctx, q, inp['uv']), _dev(ctx, q, inp['w_plane']), _dev(ctx, q, inp['vis'])
    if variant == 'binned':
        nbytes = L.kimg_grid_binned_workspace_bytes(n, P, W, OV, K)
    else:
        nbytes = L.kimg_grid_workspace_bytes(n, P, W, OV, K)
    ws, nbytes = _workspace(ctx, nbytes)
    rc = L.kimg_grid(g.dev.ptr, g.row, g.pol, G, P, wg.dev.ptr, wg.row, wg.pol, uv.ptr, wp.ptr,
                     vis.ptr, n, table.ptr, W, OV, K, ws.ptr if ws is not None else None, nbytes,
                     grid.GRID_VARIANTS[variant] | case.cus << 8,
                     grid.GRID_ARITH.get(arith, arith) | (0 if fold else NO_FOLD), q.handle)
    check(rc, 'kimg_grid %s %s fold=%s' % (variant, arith, fold))
    q.finish()
    return g.get(q)


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=repr)
def test_fold_exact(case):
    """Fold on, fold off, the oracle's grid and the float64 truth, bit for bit: every arithmetic
    form, window and binned variants."""
    from oracle import kimg_oracle as orc
    ctx, q = context_queue()
    inp, ok = fold_stream(case)
    want, bound = _truth(inp, ok)
    assert bound.max() < EXACT
    oracle = np.zeros((case.P, case.G, case.G), np.complex64)
    orc.grid(inp['kern'], oracle, inp['wg'], inp['uv'][ok][:, :2], inp['uv'][ok][:, 2:],
             inp['w_plane'][ok], inp['vis'][ok])
    _assert_exact(oracle, want, 'oracle')
    for variant in ('mfma', 'binned'):
        for arith in FORMS:
            on = _run(ctx, q, case, inp, variant, arith, True)
            off = _run(ctx, q, case, inp, variant, arith, False)
            _assert_exact(off, want, '%s/%s unfolded' % (variant, arith))
            _assert_exact(on, want, '%s/%s folded' % (variant, arith))
            assert np.array_equal(_bits(on), _bits(off)), (variant, arith)
            assert np.array_equal(_bits(on), _bits(oracle)), (variant, arith)


@pytest.mark.gpu
def test_arith_flag_is_checked():
    """The bit rides on every form; anything else in `arith` is still KIMG_EINVAL."""
    from katsdpimager_amd._lib import KimgError
    ctx, q = context_queue()
    case = CASES[0]
    inp, ok = fold_stream(case)
    for fold in (True, False):
        for arith in (3, 0x200, 0x80):
            with pytest.raises(KimgError):
                _run(ctx, q, case, inp, 'mfma', arith, fold)


def _operators(obs, P, K, n):
    from katsdpimager_amd import accel, grid
    import synth
    import torch
    ctx, q = context_queue()
    ip, gp, ap = synth.make_parameters(obs, P, K)
    fns = {}
    for fold in (True, False):
        fns[fold] = grid.GridderTemplate(ctx, ip.fixed, gp.fixed, {'variant': 'mfma', 'fold_runs': fold}) \
            .instantiate(q, ap, ip, gp, n)
    Gg = fns[True].slots['grid'].shape[1]
    gen = torch.Generator(device=ctx.device)
    gen.manual_seed(2)
    wg = accel.DeviceArray(ctx, (P, Gg, Gg), np.float32,
                           tensor=torch.rand((P, Gg, Gg), generator=gen, device=ctx.device))
    for fn in fns.values():
        fn.bind(weights_grid=wg)
        fn.ensure_all_bound()
    torch.cuda.synchronize()
    return ctx, q, fns, wg


def _fraction_of_heads(obs):
    import torch
    same = torch.all(obs.uv[1:] == obs.uv[:-1], dim=1) & (obs.w_plane[1:] == obs.w_plane[:-1])
    return 1.0 - float(same.sum()) / obs.n_vis


@pytest.mark.gpu
def test_no_duplicates_same_sums():
    """A stream without adjacent duplicates (a merged track set): every batch is all heads, the
    scalar branch takes the plain staging, every cell sees the same fmaf sequence.  The folded grid
    may differ from the unfolded one by no more than unfolded grids differ among themselves (the
    order of the float atomics): the largest difference between any two of 24 unfolded runs,
    measured first.  (24 runs, 276 pairs: folded against unfolded is one more draw from the same
    distribution when the code is right, and exceeds the largest of 276 about once in 277 times; a
    fold that changed a sum would show in every draw.)

    Measured on MI355X (4.2 M records merged to 1.9 M, five unfolded runs): folded against unfolded
    7.47e-6, unfolded run to run 7.64e-6, at a peak of 30.05 (2.5e-7 of it)."""
    import itertools
    import synth
    from test_full_size import _grid_all
    ctx, q = context_queue()
    n = 1 << 22
    obs = synth.compress_adjacent(synth.make_observation(4096, n, 32, 1, device=ctx.device))
    assert _fraction_of_heads(obs) == 1.0 and obs.n_vis > (1 << 20)
    ctx, q, fns, wg = _operators(obs, 1, 28, obs.n_vis)
    off = [_grid_all(ctx, q, obs, fns[False]).clone() for _ in range(24)]
    spread = max(float((a - b).abs().max()) for a, b in itertools.combinations(off, 2))
    on = _grid_all(ctx, q, obs, fns[True]).clone()
    diff = float((on - off[0]).abs().max())
    peak = float(off[0].abs().max())
    print('no duplicates: folded vs unfolded %.3e, unfolded run to run %.3e (peak %.3e)' % (diff, spread, peak))
    assert diff <= spread
    assert bool(((on != 0) == (off[0] != 0)).all())


@pytest.mark.gpu
def test_rounded_duplicate_heavy_stream():
    """2 M records from the middle of the 50 M-record C2 stream (uncompressed earth-rotation tracks:
    most records repeat their predecessor's sub-cell), float samples: the max-norm error of the
    folded grid against a float64 truth is at most twice that of the unfolded grid (folding sums
    fewer, larger terms; the factor covers the scan's summation order); same non-zero cells.

    Measured on MI355X: 0.1215 of the records head a run; max-norm error over the peak 2.09e-7 folded,
    1.20e-6 unfolded."""
    import synth
    from test_full_size import _grid_all
    ctx, q = context_queue()
    n, total = 1 << 21, 50_000_000
    start = total // 2
    uvw = synth.track_uvw(total, ctx.device)[start:start + n].contiguous()
    obs = synth.make_observation(4096, n, 32, 1, device=ctx.device, uvw=uvw)
    del uvw
    heads = _fraction_of_heads(obs)
    assert heads < 0.5
    ctx, q, fns, wg = _operators(obs, 1, 28, n)
    on = _grid_all(ctx, q, obs, fns[True]).clone()
    off = _grid_all(ctx, q, obs, fns[False]).clone()
    truth = synth.grid_truth_fp64(fns[True].convolve_kernel.data, obs.uv, obs.w_plane, obs.vis,
                                  wg.tensor, 28)[0]
    peak = float(truth.abs().max())
    err_on = float((on[0].to(truth.dtype) - truth).abs().max())
    err_off = float((off[0].to(truth.dtype) - truth).abs().max())
    print('rounded: heads %.4f of the records; max-norm error / peak: folded %.3e, unfolded %.3e'
          % (heads, err_on / peak, err_off / peak))
    assert err_on <= 2 * err_off
    assert bool(((on != 0) == (off != 0)).all())
