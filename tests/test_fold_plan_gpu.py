"""Fold plans (include/kimg.h: kimg_fold_plan, kimg_fold_runs_planned, kimg_grid_planned,
KIMG_ARITH_NO_PREFOLD), through the C ABI.

* kimg_fold_runs_planned writes bit for bit what kimg_fold_runs writes: the header's fields, the
  spans' counts, the compacted uv, w_plane and the float32 sums (integer-valued samples), at record
  counts that straddle a tile and a span, with one to four polarizations.
* kimg_grid_planned on integer streams: the grid of the unplanned call with KIMG_ARITH_PREFOLD, bit
  for bit, use_folded = 1 and the same count.
* Stale plans -- another stream of the same length, a uv word rewritten in place, another span
  layout, another length, a buffer of 0xFF: use_folded = 0, the grid of the unfolded gridder, and
  no byte written behind the workspace.
* KIMG_ARITH_NO_PREFOLD skips the pre-pass where the call would take it.
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
from test_exact_gridding import EXACT, _assert_exact, _bits, _dev        # noqa: E402
from test_fold_runs import FoldCase, fold_stream        # noqa: E402
from test_fold_prepass_gpu import (CANARY, COUNTS_BYTES, HEADER_BYTES, NO_FOLD, PREFOLD, TILE,      # noqa: E402
                                   _cover_bound, _cut, _truth, fold_input, fold_samples, grid_sizes,
                                   numpy_heads, parse_fold_workspace, simple_stream)

pytestmark = pytest.mark.gpu

NO_PREFOLD = 0x800                      # KIMG_ARITH_NO_PREFOLD
KIMG_EINVAL = -10001
GUARD = 4096
# one record, part of one thread's eight, a tile less one, a tile, a tile and one, three tiles (three
# spans), six spans with a partial last tile
SIZES = (1, 7, TILE - 1, TILE, TILE + 1, 3 * TILE, 5 * TILE + 17)


def make_plan(ctx, q, d_uv, d_wp, n, P):
    from katsdpimager_amd import accel
    from katsdpimager_amd._lib import check, lib
    nbytes = lib().kimg_fold_plan_bytes()
    assert nbytes >= 32 + 4 * 1024
    plan = accel.DeviceArray(ctx, (nbytes + GUARD,), np.uint8)
    plan.set(q, np.full(nbytes + GUARD, CANARY, np.uint8))
    check(lib().kimg_fold_plan(d_uv.ptr, d_wp.ptr, n, P, plan.ptr, q.handle), 'kimg_fold_plan')
    raw = plan.get(q)
    assert np.all(raw[nbytes:] == CANARY), 'written behind the plan'
    return plan, raw[:nbytes]


def plan_fields(raw):
    return dict(spans=int(raw[4:8].view(np.uint32)[0]), num_vis=int(raw[8:16].view(np.int64)[0]),
                tiles_per_span=int(raw[16:24].view(np.int64)[0]), count=int(raw[24:32].view(np.int64)[0]),
                counts=raw[64:64 + 4096].view(np.uint32))


def span_counts(uv, wp, spans, tiles_per_span):
    """Heads per span: those of the stream, and every span's first record."""
    head = numpy_heads(uv, wp)
    step = tiles_per_span * TILE
    head[::step] = True
    return np.add.reduceat(head.astype(np.int64), np.arange(0, len(head), step))[:spans]


def run_fold(ctx, q, dev, n, P, capacity, plan=None):
    """kimg_fold_runs (plan None) or kimg_fold_runs_planned -> (parsed header, workspace bytes)."""
    from katsdpimager_amd import accel
    from katsdpimager_amd._lib import check, lib
    L = lib()
    nbytes = L.kimg_fold_runs_workspace_bytes(P, capacity)
    ws = accel.DeviceArray(ctx, (nbytes + GUARD,), np.uint8)
    ws.set(q, np.full(nbytes + GUARD, CANARY, np.uint8))
    d_uv, d_wp, d_vis = dev
    if plan is None:
        rc = L.kimg_fold_runs(d_uv.ptr, d_wp.ptr, d_vis.ptr, n, P, capacity, ws.ptr, nbytes, q.handle)
    else:
        rc = L.kimg_fold_runs_planned(d_uv.ptr, d_wp.ptr, d_vis.ptr, n, P, capacity, ws.ptr, nbytes,
                                      q.handle, plan.ptr)
    check(rc, 'kimg_fold_runs')
    q.finish()
    raw = ws.get(q)
    assert np.all(raw[nbytes:] == CANARY), 'written behind the workspace'
    return parse_fold_workspace(raw[:nbytes], ws.ptr, P, capacity), raw[:nbytes]


@pytest.mark.parametrize('P', [1, 2, 3, 4])
def test_planned_fold_is_the_unplanned_fold(P):
    ctx, q = context_queue()
    rs = np.random.RandomState(60 + P)
    for n in SIZES:
        for kind in ('runs', 'exactly_half') if n >= 2 and n % 2 == 0 else ('runs',):
            uv, wp = fold_input(kind, n, rs)
            vis = fold_samples(n, P)
            dev = (_dev(ctx, q, uv), _dev(ctx, q, wp), _dev(ctx, q, vis))
            what = '%s n=%d P=%d' % (kind, n, P)
            plan, praw = make_plan(ctx, q, dev[0], dev[1], n, P)
            f = plan_fields(praw)
            assert f['num_vis'] == n and f['spans'] == -(-n // TILE) and f['tiles_per_span'] == 1, what
            want_counts = span_counts(uv, wp, f['spans'], 1)
            assert np.array_equal(f['counts'][:f['spans']], want_counts), what
            assert not f['counts'][f['spans']:].any() and f['count'] == want_counts.sum(), what
            a, araw = run_fold(ctx, q, dev, n, P, n // 2)
            b, braw = run_fold(ctx, q, dev, n, P, n // 2, plan)
            for key in ('use_folded', 'spans', 'count', 'capacity', 'sections'):
                assert a[key] == b[key], (what, key, a[key], b[key])
            assert a['count'] == f['count'] and a['use_folded'] == int(2 * a['count'] <= n), what
            counts = slice(HEADER_BYTES, HEADER_BYTES + 4 * a['spans'])
            if a['use_folded']:         # (a plan that does not fold ends the launch at once)
                assert np.array_equal(araw[counts], braw[counts]), what
            body = HEADER_BYTES + COUNTS_BYTES
            assert np.array_equal(araw[body:], braw[body:]), what       # uv, sums, w_plane, untouched bytes


def test_planned_fold_with_several_tiles_per_span():
    """More than 768 tiles: spans of two tiles, the last one partial, three polarizations on the
    layout of 512 spans; the plan's counts are the count launch's."""
    ctx, q = context_queue()
    rs = np.random.RandomState(3)
    for P, n in ((1, 769 * TILE + 5), (3, 513 * TILE + 5)):
        uv, wp = fold_input('runs', n, rs)
        vis = fold_samples(n, P)
        dev = (_dev(ctx, q, uv), _dev(ctx, q, wp), _dev(ctx, q, vis))
        plan, praw = make_plan(ctx, q, dev[0], dev[1], n, P)
        f = plan_fields(praw)
        assert f['tiles_per_span'] == 2 and f['spans'] == (385 if P == 1 else 257)
        assert np.array_equal(f['counts'][:f['spans']], span_counts(uv, wp, f['spans'], 2))
        a, araw = run_fold(ctx, q, dev, n, P, n // 2)
        b, braw = run_fold(ctx, q, dev, n, P, n // 2, plan)
        assert a['use_folded'] == b['use_folded'] == 1 and a['count'] == b['count'] == f['count']
        assert np.array_equal(araw[HEADER_BYTES:], braw[HEADER_BYTES:])


# ---------------------------------------------------------------------------------------------
# through kimg_grid

class Call:
    """The device side of one kimg_grid call on a stream: inputs uploaded once, so that a plan can be
    made on them and they can be rewritten in place."""

    def __init__(self, ctx, q, case, inp):
        from katsdpimager_amd import accel
        self.ctx, self.q, self.case, self.n = ctx, q, case, len(inp['uv'])
        self.wg = Padded(ctx, q, inp['wg'], 0, 0, np.float32(1e6))
        self.table = _dev(ctx, q, inp['kern'])
        self.uv, self.wp, self.vis = _dev(ctx, q, inp['uv']), _dev(ctx, q, inp['w_plane']), _dev(ctx, q, inp['vis'])
        self.own, self.nbytes = grid_sizes(case, self.n)
        self.ws = accel.DeviceArray(ctx, (self.nbytes + GUARD,), np.uint8)

    def plan(self, n=None, P=None):
        return make_plan(self.ctx, self.q, self.uv, self.wp, n or self.n, P or self.case.P)[0]

    def grid(self, bits, plan=None, want_rc=0):
        """-> (grid, header of the pre-pass)"""
        from katsdpimager_amd import grid
        from katsdpimager_amd._lib import check, lib
        L, c, q = lib(), self.case, self.q
        g = Padded(self.ctx, q, np.zeros((c.P, c.G, c.G), np.complex64), 3, 1, np.complex64(-1.5e7 + 3.25e6j))
        fill = np.full(self.nbytes + GUARD, CANARY, np.uint8)
        fill[:self.nbytes] = 0
        self.ws.set(q, fill)
        args = (g.dev.ptr, g.row, g.pol, c.G, c.P, self.wg.dev.ptr, self.wg.row, self.wg.pol, self.uv.ptr,
                self.wp.ptr, self.vis.ptr, self.n, self.table.ptr, c.W, c.OV, c.K, self.ws.ptr, self.nbytes,
                grid.GRID_VARIANTS['mfma'] | c.cus << 8, grid.GRID_ARITH['fp32'] | bits, q.handle)
        rc = L.kimg_grid(*args) if plan is None else L.kimg_grid_planned(*args, plan.ptr)
        if want_rc:
            assert rc == want_rc
            return None, None
        check(rc, 'kimg_grid')
        q.finish()
        raw = self.ws.get(q)
        assert np.all(raw[self.nbytes:] == CANARY), 'written behind the workspace'
        raw = raw[self.own - 256:]
        return g.get(q), dict(use_folded=int(raw[0:4].view(np.uint32)[0]), count=int(raw[8:16].view(np.int64)[0]))


GRID_CASES = [
    FoldCase('k28_p1', 28, 8, 4, 1, 5 * TILE + 17, 168),
    FoldCase('k28_p2', 28, 8, 4, 2, 3 * TILE, 168),
    FoldCase('k28_p3', 28, 8, 4, 3, TILE + 1, 168),
    FoldCase('k28_p4', 28, 8, 4, 4, TILE - 1, 168),
    FoldCase('k28_hbm_p1', 28, 8, 96, 1, TILE, 168),
]


@pytest.mark.parametrize('case', GRID_CASES, ids=repr)
def test_planned_grid_is_the_prefold_grid(case):
    ctx, q = context_queue()
    inp, ok = _cut(*fold_stream(case), case.n)
    call = Call(ctx, q, case, inp)
    want, hdr = call.grid(PREFOLD)
    assert hdr['use_folded'] == 1
    got, got_hdr = call.grid(0, call.plan())
    assert got_hdr == hdr
    assert np.array_equal(_bits(got), _bits(want))
    _assert_exact(got, _truth(inp, ok), repr(case))
    # the bit that says "does not fold": no pre-pass (the header stays as the test zeroed it)
    for bits, plan in ((NO_PREFOLD, None), (NO_PREFOLD, call.plan()), (NO_FOLD, call.plan())):
        got, got_hdr = call.grid(bits, plan)
        assert got_hdr == dict(use_folded=0, count=0)
        assert np.array_equal(_bits(got), _bits(want))
    call.grid(PREFOLD | NO_PREFOLD, want_rc=KIMG_EINVAL)


def _stale(call, plan, unfolded, what):
    got, hdr = call.grid(0, plan)
    assert hdr['use_folded'] == 0, what
    assert np.array_equal(_bits(got), _bits(unfolded)), what


@pytest.mark.parametrize('P', [1, 3])
def test_stale_plans_never_change_the_grid(P):
    from katsdpimager_amd import accel
    ctx, q = context_queue()
    n = 5 * TILE + 17
    case = FoldCase('stale_p%d' % P, 28, 8, 4, P, n, 168)
    a = simple_stream('stale_a', 28, 8, 4, P, n, 168, [2, 3, 5, 9, 30])
    b = simple_stream('stale_b', 28, 8, 4, P, n, 168, [2, 4, 7, 40, 200])
    assert not np.array_equal(span_counts(a['uv'], a['w_plane'], 6, 1), span_counts(b['uv'], b['w_plane'], 6, 1))
    call_a, call_b = Call(ctx, q, case, a), Call(ctx, q, case, b)
    unfolded, _ = call_b.grid(NO_FOLD)
    _assert_exact(unfolded, _truth(b, np.ones(n, bool)), 'unfolded')
    fresh, hdr = call_b.grid(0, call_b.plan())
    assert hdr['use_folded'] == 1 and np.array_equal(_bits(fresh), _bits(unfolded))
    # the plan of another stream of the same length
    _stale(call_b, call_a.plan(), unfolded, 'plan of stream A')
    # plans of this stream for another length and for another layout of the spans' fields
    _stale(call_b, call_b.plan(n=n - 1), unfolded, 'plan for n - 1 records')
    _stale(call_b, call_b.plan(n=3 * TILE), unfolded, 'plan for fewer spans')
    # arbitrary bytes
    junk = accel.DeviceArray(ctx, (call_b.plan().shape[0],), np.uint8)
    for byte in (0xFF, 0x00):
        junk.set(q, np.full(junk.shape, byte, np.uint8))
        _stale(call_b, junk, unfolded, 'plan of %#x bytes' % byte)
    # a misaligned plan is the one thing the host can see
    from katsdpimager_amd._lib import lib
    assert lib().kimg_fold_runs_planned(call_b.uv.ptr, call_b.wp.ptr, call_b.vis.ptr, n, P, n // 2,
                                        call_b.ws.ptr, call_b.nbytes, q.handle, junk.ptr + 8) == KIMG_EINVAL
    # one uv word rewritten in place after planning, in the middle span, inside a run: its record
    # and the next now head runs of their own
    plan = call_b.plan()
    heads = numpy_heads(b['uv'], b['w_plane'])
    inside = np.flatnonzero(~heads[:-1] & ~heads[1:])
    i = int(inside[np.searchsorted(inside, 2 * TILE + TILE // 2)])
    assert 2 * TILE < i < 3 * TILE - 1
    uv = b['uv'].copy()
    uv[i, 0] += 1
    call_b.uv.set(q, uv)
    rewritten = dict(b, uv=uv)
    unfolded, _ = call_b.grid(NO_FOLD)
    _assert_exact(unfolded, _truth(rewritten, np.ones(n, bool)), 'rewritten, unfolded')
    _stale(call_b, plan, unfolded, 'uv rewritten in place')
    # counts that are right in sum and wrong per span: the offsets would be wrong
    raw = plan.get(q)
    counts = raw[64:64 + 4096].view(np.uint32)
    counts[1] += 1
    counts[2] -= 1
    call_b.uv.set(q, b['uv'])
    plan.set(q, raw)
    unfolded, _ = call_b.grid(NO_FOLD)
    _stale(call_b, plan, unfolded, 'two counts exchanged one head')


def test_plan_for_another_polarization_layout():
    """More than 512 tiles: two polarizations cut 600 spans of one tile, three 300 spans of two.  A
    plan made for the one layout is refused by a call with the other."""
    ctx, q = context_queue()
    n, G = 600 * TILE + 5, 1024
    case = FoldCase('layout', 28, 8, 4, 2, n, G, amp=1)
    inp = simple_stream(case.name, 28, 8, 4, 2, n, G, [2, 3, 4, 5], amp=1)
    assert _cover_bound(inp, 28, G) < EXACT
    call = Call(ctx, q, case, inp)
    unfolded, _ = call.grid(NO_FOLD)
    assert np.any(unfolded != 0)
    fresh, hdr = call.grid(0, call.plan())
    assert hdr['use_folded'] == 1 and np.array_equal(_bits(fresh), _bits(unfolded))
    _stale(call, call.plan(P=3), unfolded, 'plan of the three-polarization layout')
