"""The fold pre-pass of the window gridder (csrc/grid_fold.hip; include/kimg.h: kimg_fold_runs,
KIMG_ARITH_PREFOLD), through the C ABI.

* kimg_fold_runs alone against a numpy statement of its contract.  Samples have real part 1 and a
  small integer imaginary part that depends on the record's index, so every sum is exact, the real
  part of an output record is its run's length, and the test need not know where the spans were cut.
* kimg_grid with KIMG_ARITH_PREFOLD against KIMG_ARITH_NO_FOLD, the default and a float64 truth, bit
  for bit on integer-valued streams (the premise of test_exact_gridding.py, asserted per case).
* float data: the pre-pass is no further from a float64 truth than the unfolded gridder.
* a case in which the folded count selects another chunk plan than the host's length would.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from helpers import Padded, context_queue        # noqa: E402
from test_exact_gridding import (EXACT, _assert_exact, _bits, _cint, _crop,     # noqa: E402
                                 _density, _dev, _table, _walk, grid_truth)
from test_fold_runs import FoldCase, fold_stream        # noqa: E402

pytestmark = pytest.mark.gpu

NO_FOLD, PREFOLD = 0x100, 0x400         # KIMG_ARITH_NO_FOLD, KIMG_ARITH_PREFOLD
KIMG_EINVAL = -10001
TILE = 256 * 8                          # records of one tile of the pre-pass
SIZES = (1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 5 * TILE + 17, 300001)
FORMS = ('fp32', 'fp32_32x32', 'split_fp16')
CANARY = 0xA5
HEADER_BYTES, COUNTS_BYTES = 256, 4096  # the workspace's first two sections (grid_fold.hip)


# ---------------------------------------------------------------------------------------------
# kimg_fold_runs alone

def _keys_from_runs(rs, lengths, n):
    """uv [n][4], w_plane [n]: one key per run, never equal to its predecessor's."""
    lengths = np.asarray(lengths)
    m = len(lengths)
    key = rs.randint(-300, 300, (m, 5))
    key[:, 4] = np.arange(m) % 50           # neighbouring runs always differ
    rec = np.repeat(key, lengths, axis=0)[:n]
    assert len(rec) == n
    return rec[:, :4].astype(np.int16), rec[:, 4].astype(np.int16)


def fold_input(kind, n, rs):
    if kind == 'runs':
        lengths = rs.permutation(np.tile(np.arange(1, 201), -(-n // 20100) + 1))
    elif kind == 'long_run':            # one run longer than a whole span (of one tile at these sizes)
        lengths = np.array([max(n // 3, 1), 3 * TILE + 5] + [2] * n)
    elif kind == 'all_equal':
        lengths = np.array([n])
    elif kind == 'no_adjacent_equal':
        lengths = np.ones(n, np.int64)
    elif kind == 'exactly_half':        # n even: 2 H == N, and no run straddles a tile
        lengths = np.full(n // 2, 2)
    elif kind == 'half_plus_one':
        lengths = np.concatenate([[1, 1], np.full(n // 2 - 1, 2)])
    else:
        raise ValueError(kind)
    return _keys_from_runs(rs, lengths, n)


def fold_samples(n, P):
    i = np.arange(n)[:, None]
    p = np.arange(P)[None, :]
    return (1 + 1j * ((i * (p + 1)) % 7 - 3)).astype(np.complex64)


def numpy_heads(uv, wp):
    key = np.concatenate([uv.astype(np.int64), wp.astype(np.int64)[:, None]], axis=1)
    head = np.ones(len(key), bool)
    head[1:] = np.any(key[1:] != key[:-1], axis=1)
    return head


def run_fold(ctx, q, uv, wp, vis, capacity):
    """-> (header dict, uv', w_plane', vis' as far as the capacity goes, the whole workspace)."""
    from katsdpimager_amd import accel
    from katsdpimager_amd._lib import check, lib
    L = lib()
    n, P = vis.shape
    nbytes = L.kimg_fold_runs_workspace_bytes(P, capacity)
    assert nbytes >= HEADER_BYTES + COUNTS_BYTES + capacity * (8 + 2 + 8 * P)
    guard = 4096
    ws = accel.DeviceArray(ctx, (nbytes + guard,), np.uint8)
    ws.set(q, np.full(nbytes + guard, CANARY, np.uint8))
    d_uv, d_wp, d_vis = _dev(ctx, q, uv), _dev(ctx, q, wp), _dev(ctx, q, vis)
    check(L.kimg_fold_runs(d_uv.ptr, d_wp.ptr, d_vis.ptr, n, P, capacity, ws.ptr, nbytes, q.handle),
          'kimg_fold_runs')
    q.finish()
    raw = ws.get(q)
    assert np.all(raw[nbytes:] == CANARY), 'written behind the workspace'
    return parse_fold_workspace(raw[:nbytes], ws.ptr, P, capacity), raw[:nbytes]


def parse_fold_workspace(raw, base, P, capacity):
    hdr = dict(use_folded=int(raw[0:4].view(np.uint32)[0]), spans=int(raw[4:8].view(np.uint32)[0]),
               count=int(raw[8:16].view(np.int64)[0]), capacity=int(raw[40:48].view(np.int64)[0]))
    off = [int(x) - base for x in raw[16:40].view(np.uint64)]
    assert hdr['capacity'] == capacity
    assert HEADER_BYTES + COUNTS_BYTES <= off[0] and off[0] + 8 * capacity <= len(raw)
    assert off[1] + 2 * capacity <= len(raw) and off[2] + 8 * P * capacity <= len(raw)
    hdr['sections'] = [(off[0], 8 * capacity), (off[1], 2 * capacity), (off[2], 8 * P * capacity)]
    hdr['uv'] = raw[off[0]:off[0] + 8 * capacity].view(np.int16).reshape(capacity, 4)
    hdr['w_plane'] = raw[off[1]:off[1] + 2 * capacity].view(np.int16)
    hdr['vis'] = raw[off[2]:off[2] + 8 * P * capacity].view(np.complex64).reshape(capacity, P)
    return hdr


def check_fold(uv, wp, vis, capacity, hdr, raw, what):
    n, P = vis.shape
    heads_min = int(numpy_heads(uv, wp).sum())
    H, spans = hdr['count'], hdr['spans']
    assert 1 <= spans <= 1024, what
    assert heads_min <= H <= heads_min + spans - 1, (what, heads_min, H, spans)
    use = 2 * H <= n and H <= capacity
    assert hdr['use_folded'] == int(use), (what, H, n, capacity)
    body = raw[HEADER_BYTES + COUNTS_BYTES:]
    if not use:
        assert np.all(body == CANARY), what + ': records written although use_folded is 0'
        return
    o_uv, o_wp, o_vis = hdr['uv'][:H], hdr['w_plane'][:H], hdr['vis'][:H]
    # nothing behind the H records of any section
    for (start, size), used in zip(hdr['sections'], (8 * H, 2 * H, 8 * P * H)):
        assert np.all(raw[start + used:start + size] == CANARY), what
    lengths = o_vis[:, 0].real.astype(np.int64)
    assert np.all(o_vis[:, 0].real == lengths) and np.all(lengths >= 1), what
    assert lengths.sum() == n, what          # consecutive segments that cover the input
    starts = np.cumsum(lengths) - lengths
    assert np.array_equal(np.repeat(o_uv, lengths, axis=0), uv), what       # one key per segment
    assert np.array_equal(np.repeat(o_wp, lengths), wp), what
    sums = np.add.reduceat(vis.astype(np.complex128), starts, axis=0)
    assert np.array_equal(o_vis.astype(np.complex128), sums), what          # exact
    same = np.all(o_uv[1:] == o_uv[:-1], axis=1) & (o_wp[1:] == o_wp[:-1])
    assert same.sum() <= spans - 1, what
    assert same.sum() == H - heads_min, what


@pytest.mark.parametrize('P', [1, 2, 3, 4])
def test_fold_runs_contract(P):
    """Every kind of stream at every length of SIZES.  SIZES already holds what three polarizations
    need: lengths that are no multiple of 8 (63, 65, TILE - 1, TILE + 1, 5 TILE + 17, 300001), whose
    last thread takes the clamped single loads of fold_load_samples, and TILE = 8 * 256 records
    exactly, where every thread of one tile takes the 16-byte loads -- which at P = 3 (records of 24
    bytes) straddle record boundaries -- and none the tail."""
    assert any(n % 8 for n in SIZES) and 8 * 256 in SIZES
    ctx, q = context_queue()
    rs = np.random.RandomState(40 + P)
    for n in SIZES:
        kinds = ['runs', 'long_run', 'all_equal', 'no_adjacent_equal']
        if n >= 2:
            kinds += ['exactly_half', 'half_plus_one']
        for kind in kinds:
            m = n - n % 2 if kind in ('exactly_half', 'half_plus_one') else n
            uv, wp = fold_input(kind, m, rs)
            vis = fold_samples(m, P)
            hdr, raw = run_fold(ctx, q, uv, wp, vis, m // 2)
            what = '%s n=%d P=%d' % (kind, m, P)
            check_fold(uv, wp, vis, m // 2, hdr, raw, what)
            if kind == 'exactly_half':
                assert hdr['use_folded'] == 1 and hdr['count'] == m // 2, what
            if kind in ('half_plus_one', 'no_adjacent_equal'):
                assert hdr['use_folded'] == 0, what
            if kind == 'all_equal' and m >= 2:
                assert hdr['use_folded'] == 1, what


@pytest.mark.parametrize('P', [1, 2, 3, 4])
def test_fold_runs_respects_the_capacity(P):
    """An output capacity below H: use_folded = 0 and nothing written, behind the capacity or before."""
    ctx, q = context_queue()
    rs = np.random.RandomState(7)
    for n in (TILE + 1, 5 * TILE + 17):
        uv, wp = fold_input('runs', n, rs)
        vis = fold_samples(n, P)
        H = int(numpy_heads(uv, wp).sum())
        assert 2 * H <= n
        for capacity in (H - 1, H // 2, 0):
            hdr, raw = run_fold(ctx, q, uv, wp, vis, capacity)
            check_fold(uv, wp, vis, capacity, hdr, raw, 'capacity %d of %d' % (capacity, H))
            assert hdr['use_folded'] == 0
        hdr, raw = run_fold(ctx, q, uv, wp, vis, H + 8)       # (up to 5 cuts at span boundaries)
        check_fold(uv, wp, vis, H + 8, hdr, raw, 'capacity H + 8')
        assert hdr['use_folded'] == 1


def several_tiles_per_span(P):
    """A length at which every span of the pre-pass has three tiles or more (it cuts at most 768
    spans, 512 for more than two polarizations)."""
    return (768 if P <= 2 else 512) * TILE * 3 + 5000


def long_lengths(rs, n, giant=20000):
    """Mostly short runs, some of 200, some of 5000 (two or three tiles of one span), one of 20 000
    (more than two whole spans of four tiles)."""
    lengths = rs.choice([1, 2, 3, 5, 9, 40, 200, 5000], n // 40, p=[.1, .2, .2, .2, .15, .1, .04, .01])
    lengths[10] = giant
    assert lengths.sum() >= n
    return lengths


@pytest.mark.parametrize('P', [1, 2, 3, 4])
def test_fold_runs_spans_of_several_tiles(P):
    """Spans of four tiles: the output offset and the open run carried from tile to tile, the scan's
    LDS totals used a third and fourth time, the prefetched tile (P = 1) handed on; P = 3 and 4
    take the plan of 512 spans without the prefetch."""
    ctx, q = context_queue()
    rs = np.random.RandomState(90 + P)
    n = several_tiles_per_span(P)
    lengths = long_lengths(rs, n)
    uv, wp = _keys_from_runs(rs, lengths, n)
    starts = np.cumsum(lengths) - lengths
    inside = starts[(lengths == 5000) & (starts + 5000 <= n)]
    assert np.any(inside // TILE + 2 <= (inside + 4999) // TILE)     # a run over three tiles
    vis = fold_samples(n, P)
    hdr, raw = run_fold(ctx, q, uv, wp, vis, n // 2)
    assert hdr['spans'] * 3 * TILE <= n
    check_fold(uv, wp, vis, n // 2, hdr, raw, 'several tiles per span, P=%d' % P)
    assert hdr['use_folded'] == 1


# ---------------------------------------------------------------------------------------------
# kimg_grid with the pre-pass

def simple_stream(name, K, OV, W, P, n, G, run_lengths, amp=1, lengths=None, track=200):
    """Runs of the given lengths (drawn from run_lengths, or `lengths` as they are) along slow
    tracks; integer-valued inputs."""
    rs = np.random.RandomState(sum(map(ord, name)))
    M = G - K
    bias = (K - 1) // 2 - G // 2
    if lengths is None:
        lengths = rs.choice(run_lengths, n)
    lengths = lengths[:int(np.searchsorted(np.cumsum(lengths), n)) + 1]
    m = len(lengths)
    pos = _walk(rs, m, M, track=track)      # tracks of `track` runs, each from a random place
    key = np.concatenate([pos + bias, rs.randint(0, OV, (m, 2)), rs.randint(0, W, (m, 1))], axis=1)
    assert OV % 2 == 0
    key[:, 2] = 2 * rs.randint(0, OV // 2, m) + np.arange(m) % 2    # neighbouring runs always differ
    rec = np.repeat(key, lengths, axis=0)[:n]
    return dict(kern=_table(rs, W, OV, K), uv=rec[:, :4].astype(np.int16), w_plane=rec[:, 4].astype(np.int16),
                vis=_cint(rs, (n, P), amp), wg=_density(rs, P, G))


def _cut(inp, ok, n):
    out = dict(inp)
    for k in ('uv', 'w_plane', 'vis'):
        out[k] = inp[k][:n]
    return out, ok[:n]


def _truth(inp, ok):
    canvas, bound = grid_truth(inp['kern'], inp['uv'][ok], inp['w_plane'][ok], inp['vis'][ok], inp['wg'])
    assert bound.max() < EXACT
    return _crop(canvas)


def _truth_of_runs(inp, bound=True):
    """The same truth at a tenth of the cost for a long stream without out-of-range records: runs
    summed first, in float64 (exact on these integers).  The bound comes from the runs' sums of
    |Re| and |Im|, which bound the partial sums of every order, folded or not."""
    starts = np.flatnonzero(numpy_heads(inp['uv'], inp['w_plane']))
    vis = inp['vis'].astype(np.complex128)
    sums = np.add.reduceat(vis, starts, axis=0)
    mags = np.add.reduceat(np.abs(vis.real) + 1j * np.abs(vis.imag), starts, axis=0)
    uv, wp = inp['uv'][starts], inp['w_plane'][starts]
    canvas, _ = grid_truth(inp['kern'], uv, wp, sums, inp['wg'])
    if bound:
        assert grid_truth(inp['kern'], uv, wp, mags, inp['wg'])[1].max() < EXACT
    return _crop(canvas)


def grid_sizes(case, n):
    from katsdpimager_amd._lib import lib
    L = lib()
    own = L.kimg_grid_workspace_bytes(0, case.P, case.W, case.OV, case.K)
    return own, own + L.kimg_fold_runs_workspace_bytes(case.P, n // 2)


def run_grid(ctx, q, case, inp, arith, bits, room='room', ws=None, want_rc=0):
    """One kimg_grid call.  room: 'room' (workspace with room for the pre-pass), 'today' (the size of
    before the pre-pass existed) or 'null'.  Returns (grid, the pre-pass's header or None)."""
    from katsdpimager_amd import accel, grid
    from katsdpimager_amd._lib import check, lib
    L = lib()
    P, G, K, W, OV = case.P, case.G, case.K, case.W, case.OV
    n = len(inp['uv'])
    g = Padded(ctx, q, np.zeros((P, G, G), np.complex64), 3, 1, np.complex64(-1.5e7 + 3.25e6j))
    wg = Padded(ctx, q, inp['wg'], 0, 0, np.float32(1e6))
    table = _dev(ctx, q, inp['kern'])
    uv, wp, vis = _dev(ctx, q, inp['uv']), _dev(ctx, q, inp['w_plane']), _dev(ctx, q, inp['vis'])
    own, with_room = grid_sizes(case, n)
    nbytes = {'room': with_room, 'today': own, 'null': 0}[room]
    if ws is None and nbytes:
        ws = accel.DeviceArray(ctx, (nbytes,), np.uint8)
        ws.zero(q)
    rc = L.kimg_grid(g.dev.ptr, g.row, g.pol, G, P, wg.dev.ptr, wg.row, wg.pol, uv.ptr, wp.ptr,
                     vis.ptr, n, table.ptr, W, OV, K, ws.ptr if nbytes else None, nbytes,
                     grid.GRID_VARIANTS['mfma'] | case.cus << 8, grid.GRID_ARITH[arith] | bits, q.handle)
    if want_rc:
        assert rc == want_rc
        return None, None
    check(rc, 'kimg_grid %s %#x %s' % (arith, bits, room))
    q.finish()
    hdr = None
    if room == 'room':
        raw = ws.get(q)[own - 256:]
        hdr = dict(use_folded=int(raw[0:4].view(np.uint32)[0]), count=int(raw[8:16].view(np.int64)[0]))
    return g.get(q), hdr


def check_case(case, inp, ok, forms=FORMS, folds=True, want=None):
    ctx, q = context_queue()
    want = _truth(inp, ok) if want is None else want
    n = len(inp['uv'])
    for arith in forms:
        what = '%r n=%d %s' % (case, n, arith)
        pre, hdr = run_grid(ctx, q, case, inp, arith, PREFOLD)
        off, _ = run_grid(ctx, q, case, inp, arith, NO_FOLD)
        on, _ = run_grid(ctx, q, case, inp, arith, 0, room='today')
        assert hdr['use_folded'] == int(folds), (what, hdr)
        if folds:
            assert hdr['count'] <= n // 2, (what, hdr)
        _assert_exact(pre, want, what + ' pre-pass')
        _assert_exact(off, want, what + ' unfolded')
        assert np.array_equal(_bits(pre), _bits(off)), what
        assert np.array_equal(_bits(pre), _bits(on)), what


GRID_CASES = [
    FoldCase('k28_p1', 28, 8, 4, 1, 6000, 168),
    FoldCase('k28_p2', 28, 8, 4, 2, 5 * TILE + 17, 168),
    FoldCase('k28_p3', 28, 8, 4, 3, 6000, 168),         # (k28_p1 with three polarizations)
    FoldCase('k28_p4', 28, 8, 4, 4, TILE + 1, 168),
    FoldCase('k40_p1', 40, 8, 4, 1, 5000, 200),
    FoldCase('k40_p3', 40, 8, 4, 3, TILE, 200),
    FoldCase('k28_hbm_p1', 28, 8, 96, 1, 6000, 168),
    FoldCase('k28_hbm_p4', 28, 8, 96, 4, TILE - 1, 168),
]


@pytest.mark.parametrize('case', GRID_CASES, ids=repr)
def test_grid_prefold_exact(case):
    """Runs of 1 .. 200 records, runs that cancel, runs interrupted by out-of-range records
    (test_fold_runs.fold_stream), cut to the case's N: every form, the pre-pass against the unfolded
    gridder, the default and the truth."""
    inp, ok = _cut(*fold_stream(case), case.n)
    assert (~ok).sum() >= 2
    check_case(case, inp, ok)


def test_grid_prefold_sizes():
    """Every N of the list (the short ones fall back inside the call when folding does not halve them)."""
    case = FoldCase('sizes', 28, 8, 4, 1, 11000, 168, amp=1)
    full, ok_full = fold_stream(case)
    for n in SIZES[:-1]:
        inp, ok = _cut(full, ok_full, n)
        assert len(inp['uv']) == n
        heads = int(numpy_heads(inp['uv'], inp['w_plane']).sum())
        check_case(case, inp, ok, forms=('fp32',), folds=2 * heads <= n)
    big = FoldCase('sizes_big', 28, 8, 4, 1, SIZES[-1], 512)
    inp = simple_stream(big.name, 28, 8, 4, 1, SIZES[-1], 512, [1, 2, 5, 9, 14, 30])
    check_case(big, inp, np.ones(SIZES[-1], bool), forms=('fp32',), want=_truth_of_runs(inp))


def test_grid_prefold_spans_of_several_tiles():
    """Two polarizations (the compaction kernel without its prefetch) at a length where every span
    has four tiles."""
    n = several_tiles_per_span(2)
    case = FoldCase('several_tiles', 28, 8, 4, 2, n, 1024)
    # (no run of 20 000 here: that many records on one cell break the exactness premise; fewer short
    # runs than long_lengths draws: the truth costs a second per 15 000 runs)
    lengths = np.random.RandomState(5).choice([5, 9, 40, 200, 5000], n // 40, p=[.2, .25, .35, .19, .01])
    inp = simple_stream(case.name, 28, 8, 4, 2, n, 1024, None, lengths=lengths, track=10)
    check_case(case, inp, np.ones(n, bool), forms=('fp32',), want=_truth_of_runs(inp))


def test_grid_prefold_without_duplicates():
    """No two adjacent records equal: the pre-pass says so in its header, the window kernel grids the
    stream as given."""
    case = FoldCase('nodup', 28, 8, 4, 2, 3 * TILE + 5, 168)
    inp = simple_stream(case.name, 28, 8, 4, 2, case.n, 168, [1])
    assert numpy_heads(inp['uv'], inp['w_plane']).all()
    check_case(case, inp, np.ones(case.n, bool), folds=False)


def test_grid_prefold_needs_room():
    """A workspace of the size of before the pre-pass existed, or none: the bit is accepted, the
    pre-pass skipped, the result the same."""
    ctx, q = context_queue()
    case = GRID_CASES[0]
    inp, ok = _cut(*fold_stream(case), case.n)
    want = _truth(inp, ok)
    for room in ('today', 'null'):
        got, _ = run_grid(ctx, q, case, inp, 'fp32', PREFOLD, room=room)
        _assert_exact(got, want, room)


def test_grid_prefold_header_does_not_leak():
    """Two calls on one workspace, the second shorter and without duplicates, then a third without the
    pre-pass: each grids its own stream."""
    from katsdpimager_amd import accel
    ctx, q = context_queue()
    case = GRID_CASES[0]
    first, ok = _cut(*fold_stream(case), case.n)
    second = simple_stream('leak', 28, 8, 4, 1, 1500, 168, [1])
    third = simple_stream('leak3', 28, 8, 4, 1, 900, 168, [3, 4])
    ws = accel.DeviceArray(ctx, (grid_sizes(case, case.n)[1],), np.uint8)
    ws.zero(q)
    for inp, mask, bits, room in ((first, ok, PREFOLD, 'room'), (second, None, PREFOLD, 'room'),
                                  (third, None, 0, 'today'), (third, None, PREFOLD, 'room')):
        mask = np.ones(len(inp['uv']), bool) if mask is None else mask
        got, _ = run_grid(ctx, q, case, inp, 'fp32', bits, room=room, ws=ws)
        _assert_exact(got, _truth(inp, mask), 'n=%d' % len(inp['uv']))


def test_prefold_with_no_fold_is_invalid():
    ctx, q = context_queue()
    case = GRID_CASES[0]
    inp, ok = _cut(*fold_stream(case), 500)
    for arith in FORMS:
        run_grid(ctx, q, case, inp, arith, PREFOLD | NO_FOLD, want_rc=KIMG_EINVAL)


@pytest.mark.parametrize('name,n,runs', [('by_the_chunk', 60000, [2, 3, 4]), ('one_span', 40000, [5, 9, 14, 30])])
def test_device_count_selects_another_plan(name, n, runs):
    """On one CU (KIMG_WINDOW_CUS(1): 2 workgroups, 24 waves) the host plans 60 000 records as 134
    chunks of 448; the ~20 000 folded records are 45 chunks to the device.  40 000 records in longer
    runs are 90 chunks to the host and too few for chunks on the device, which goes back to one span
    per workgroup.  What this shows is that a stream divided otherwise than the host planned is
    still gridded whole; it cannot tell a stale chunk length or multiplier (both plans choose 448 and
    7919 here): test_device_multiplier_is_coprime_to_the_device_count does that."""
    case = FoldCase(name, 28, 8, 4, 1, n, 256, cus=1)
    inp = simple_stream(name, 28, 8, 4, 1, n, 256, runs)
    heads = int(numpy_heads(inp['uv'], inp['w_plane']).sum())
    waves, min_chunk = 24, 384
    assert n // (waves * min_chunk) >= 2
    if name == 'by_the_chunk':
        assert 2 * heads <= n and heads // (waves * min_chunk) >= 2
        assert heads // (waves * min_chunk) != n // (waves * min_chunk)
    else:
        assert heads // (waves * min_chunk) < 2
    check_case(case, inp, np.ones(n, bool), forms=('fp32', 'split_fp16'))


def _chunk_count(n, waves, min_chunk=384, max_parts=16):
    """Chunks of a launch of `waves` waves over n records (csrc/kimg_window_plan.h), 0: none."""
    parts = min(max_parts, n // (waves * min_chunk))
    if parts < 2:
        return 0
    chunk = -(-(-(-n // (waves * parts))) // 64) * 64
    return -(-n // chunk)


def _cover_bound(inp, K, G):
    """An upper bound of the exactness premise without the truth: per cell, the records whose
    footprint covers it, each with |Re| + |Im| of its sample, times the largest weight (3) and the
    largest |Re| + |Im| of a tap (14) squared."""
    bias = (K - 1) // 2 - G // 2
    x = inp['uv'][:, 0].astype(np.int64) - bias
    y = inp['uv'][:, 1].astype(np.int64) - bias
    mag = (np.abs(inp['vis'].real) + np.abs(inp['vis'].imag)).max(axis=1).astype(np.float64)
    at = np.bincount(y * G + x, weights=mag, minlength=G * G).reshape(G, G)
    c = np.cumsum(np.cumsum(np.pad(at, ((K, 0), (K, 0))), axis=0), axis=1)
    box = c[K:, K:] - c[:-K, K:] - c[K:, :-K] + c[:-K, :-K]         # footprints reaching back K cells
    return box.max() * 3 * 14 * 14


def test_device_multiplier_is_coprime_to_the_device_count():
    """The one place where the device's plan can silently grid wrongly.  On 21 CUs (42 workgroups of
    12 waves) 8 870 688 records are 7701 chunks to the host, which takes the multiplier 7919; they
    fold to 3 547 489 records, 7919 chunks of 448 to the device.  With the host's multiplier every
    ticket would be chunk 0.  Runs of 2 and 3 that fill every tile of the pre-pass exactly (409 of 2
    and 410 of 3), so that no span boundary cuts a run and the folded count is known; compared bit
    for bit with the unfolded gridder (the exactness premise bounded from above without a truth: a
    float64 truth of 7 G terms would take minutes)."""
    ctx, q = context_queue()
    rs = np.random.RandomState(11)
    tiles, NW, cus, G = 4331, 12, 21, 2048
    per_tile = np.array([2] * 409 + [3] * 410)
    assert per_tile.sum() == TILE
    lengths = np.concatenate([rs.permutation(per_tile) for _ in range(8)] * (tiles // 8 + 1))[:819 * tiles]
    lengths = np.concatenate([lengths, np.full(400, 2)])
    n, heads = int(lengths.sum()), len(lengths)
    case = FoldCase('coprime', 28, 8, 4, 1, n, G, cus=cus)
    inp = simple_stream(case.name, 28, 8, 4, 1, n, G, None, lengths=lengths)
    assert int(numpy_heads(inp['uv'], inp['w_plane']).sum()) == heads and 2 * heads <= n
    # the host's plan for n records and the device's for the folded ones, with the host's workgroups
    per_block = max(-(-(-(-n // (2 * cus))) // 64) * 64, 64 * NW)
    waves = -(-n // per_block) * NW
    assert waves == 2 * cus * NW
    assert _chunk_count(n, waves) % 7919 != 0 and _chunk_count(heads, waves) == 7919
    assert _cover_bound(inp, 28, G) < EXACT
    pre, hdr = run_grid(ctx, q, case, inp, 'fp32', PREFOLD)
    assert hdr == dict(use_folded=1, count=heads)
    off, _ = run_grid(ctx, q, case, inp, 'fp32', NO_FOLD)
    assert np.any(off != 0)
    assert np.array_equal(_bits(pre), _bits(off))


# ---------------------------------------------------------------------------------------------
# float data

def test_prefold_rounded_duplicate_heavy_stream():
    """2 M records from the middle of the 50 M-record C2 stream, float samples: the max-norm error
    against a float64 truth, over the peak, with the pre-pass is no larger than the unfolded
    gridder's own on the same records (the pre-pass sums fewer, larger terms)."""
    import synth
    import torch
    from katsdpimager_amd import accel, grid
    from katsdpimager_amd._lib import lib
    from test_full_size import _grid_all
    ctx, q = context_queue()
    n, total = 1 << 21, 50_000_000
    start = total // 2
    uvw = synth.track_uvw(total, ctx.device)[start:start + n].contiguous()
    obs = synth.make_observation(4096, n, 32, 1, device=ctx.device, uvw=uvw)
    del uvw
    ip, gp, ap = synth.make_parameters(obs, 1, 28)
    fns = {}
    for fold in (True, False):
        fns[fold] = grid.GridderTemplate(ctx, ip.fixed, gp.fixed, {'variant': 'mfma', 'fold_runs': fold}) \
            .instantiate(q, ap, ip, gp, n)
    pre = fns[True]
    pre.template.arith |= PREFOLD
    table = pre.convolve_kernel.padded_data
    nbytes = lib().kimg_grid_workspace_bytes(0, 1, *table.shape) + lib().kimg_fold_runs_workspace_bytes(1, n // 2)
    pre._workspace = accel.DeviceArray(ctx, (nbytes,), np.uint8, queue=q)
    pre._workspace_bytes = nbytes
    Gg = pre.slots['grid'].shape[1]
    gen = torch.Generator(device=ctx.device)
    gen.manual_seed(2)
    wg = accel.DeviceArray(ctx, (1, Gg, Gg), np.float32,
                           tensor=torch.rand((1, Gg, Gg), generator=gen, device=ctx.device))
    for fn in fns.values():
        fn.bind(weights_grid=wg)
        fn.ensure_all_bound()
    torch.cuda.synchronize()
    on = _grid_all(ctx, q, obs, pre).clone()
    hdr = pre._workspace.get(q)[nbytes - 256 - lib().kimg_fold_runs_workspace_bytes(1, n // 2):][:16]
    assert int(hdr[0:4].view(np.uint32)[0]) == 1 and int(hdr[8:16].view(np.int64)[0]) < n // 4
    off = _grid_all(ctx, q, obs, fns[False]).clone()
    truth = synth.grid_truth_fp64(pre.convolve_kernel.data, obs.uv, obs.w_plane, obs.vis, wg.tensor, 28)[0]
    peak = float(truth.abs().max())
    err_on = float((on[0].to(truth.dtype) - truth).abs().max()) / peak
    err_off = float((off[0].to(truth.dtype) - truth).abs().max()) / peak
    print('pre-pass: max-norm error / peak %.3e, unfolded %.3e' % (err_on, err_off))
    assert err_on <= err_off
    assert bool(((on != 0) == (off != 0)).all())
