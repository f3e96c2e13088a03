"""Fold maps (include/kimg.h: kimg_fold_map_bytes, kimg_fold_map, kimg_fold_runs_mapped,
kimg_grid_mapped), through the C ABI.

* A map's contents against numpy: the spans' counts, H, every thread's head bits (a span's first
  record always set), the compacted uv and w_plane; nothing written behind the map.
* kimg_fold_runs_mapped against kimg_fold_runs_planned on NON-INTEGER float samples: the header's
  count and use_folded and the sums bit for bit, the map's coordinates equal to the planned call's.
* kimg_grid_mapped against kimg_grid_planned on integer streams, bit for bit.
* Refused maps -- another length, another polarization layout, 0xFF bytes, a map made from another
  stream's plan (valid = 0), H above the capacity: use_folded = 0, the unfolded grid, nothing written
  behind the workspace.
* A valid header over head bits that are all set: the calls complete and write nothing behind the
  capacity or the workspace.
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
from test_fold_prepass_gpu import (CANARY, COUNTS_BYTES, HEADER_BYTES, NO_FOLD, TILE,      # noqa: E402
                                   _cover_bound, _cut, _truth, fold_input, numpy_heads, simple_stream)
from test_fold_plan_gpu import (GRID_CASES, GUARD, SIZES, Call, make_plan, plan_fields,      # noqa: E402
                                run_fold, span_counts)

pytestmark = pytest.mark.gpu

MAP_HEADER = 64 + 4096                  # kimg_fold_map_data: 64 bytes, then one count per span
MAP_MAGIC = 0x314d4c46
# (P, N) of test_planned_fold_with_several_tiles_per_span: spans of two tiles, the last one partial
SEVERAL = ((1, 769 * TILE + 5), (3, 513 * TILE + 5))


def map_layout(n, H):
    """Byte offsets of a map's head bits, uv and w_plane, and its end."""
    bits = MAP_HEADER
    uv = bits + (-(-n // 8) + 15) // 16 * 16
    w = uv + 8 * (-(-H // 8) * 8)
    return bits, uv, w, w + 2 * (-(-H // 8) * 8)


def map_fields(raw):
    return dict(magic=int(raw[0:4].view(np.uint32)[0]), spans=int(raw[4:8].view(np.uint32)[0]),
                num_vis=int(raw[8:16].view(np.int64)[0]), tiles_per_span=int(raw[16:24].view(np.int64)[0]),
                count=int(raw[24:32].view(np.int64)[0]), heads=int(raw[32:40].view(np.int64)[0]),
                valid=int(raw[40:44].view(np.uint32)[0]), counts=raw[64:64 + 4096].view(np.uint32))


def make_map(ctx, q, d_uv, d_wp, n, P, plan, heads):
    """kimg_fold_map into a buffer of exactly kimg_fold_map_bytes(n, P, heads) with a guard behind it
    -> (device buffer, its bytes)."""
    from katsdpimager_amd import accel
    from katsdpimager_amd._lib import check, lib
    nbytes = lib().kimg_fold_map_bytes(n, P, heads)
    assert nbytes == map_layout(n, heads)[3] and nbytes % 16 == 0
    buf = accel.DeviceArray(ctx, (nbytes + GUARD,), np.uint8)
    buf.set(q, np.full(nbytes + GUARD, CANARY, np.uint8))
    check(lib().kimg_fold_map(d_uv.ptr, d_wp.ptr, n, P, plan.ptr, buf.ptr, nbytes, q.handle), 'kimg_fold_map')
    q.finish()
    raw = buf.get(q)
    assert np.all(raw[nbytes:] == CANARY), 'written behind the map'
    return buf, raw[:nbytes]


def planned_map(ctx, q, d_uv, d_wp, n, P):
    plan, praw = make_plan(ctx, q, d_uv, d_wp, n, P)
    f = plan_fields(praw)
    buf, raw = make_map(ctx, q, d_uv, d_wp, n, P, plan, f['count'])
    return plan, f, buf, raw


def span_heads(uv, wp, tiles_per_span):
    head = numpy_heads(uv, wp)
    head[::tiles_per_span * TILE] = True
    return head


def check_map(raw, uv, wp, f, what):
    """The map `raw` of the stream (uv, wp) whose plan has the fields `f`."""
    n = len(uv)
    m = map_fields(raw)
    head = span_heads(uv, wp, f['tiles_per_span'])
    H = int(head.sum())
    assert (m['magic'], m['valid'], m['num_vis'], m['spans'], m['tiles_per_span'], m['count']) \
        == (MAP_MAGIC, 1, n, f['spans'], f['tiles_per_span'], H), (what, m)
    assert m['heads'] >= H and f['count'] == H, what
    assert np.array_equal(m['counts'][:m['spans']], span_counts(uv, wp, m['spans'], m['tiles_per_span'])), what
    assert not m['counts'][m['spans']:].any(), what
    bits, o_uv, o_w, end = map_layout(n, H)
    assert end == len(raw), what
    want_bits = np.packbits(np.pad(head, (0, -n % 8)), bitorder='little')
    assert np.array_equal(raw[bits:bits + len(want_bits)], want_bits), what
    assert np.all(raw[bits + len(want_bits):o_uv] == CANARY), what      # (the padding is nobody's)
    assert np.array_equal(raw[o_uv:o_uv + 8 * H].view(np.int16).reshape(H, 4), uv[head]), what
    assert np.array_equal(raw[o_w:o_w + 2 * H].view(np.int16), wp[head]), what
    assert np.all(raw[o_uv + 8 * H:o_w] == CANARY) and np.all(raw[o_w + 2 * H:] == CANARY), what


def float_samples(rs, n, P):
    """Samples whose sums round: the order of the additions shows in the last bits."""
    v = (rs.standard_normal((n, P)) + 1j * rs.standard_normal((n, P))) * 10.0 ** rs.randint(-3, 4, (n, 1))
    return v.astype(np.complex64)


def run_mapped(ctx, q, dev, n, P, capacity, fmap):
    """kimg_fold_runs_mapped -> (header fields, pointer offsets, the workspace's bytes)."""
    from katsdpimager_amd import accel
    from katsdpimager_amd._lib import check, lib
    L = lib()
    nbytes = L.kimg_fold_runs_workspace_bytes(P, capacity)
    ws = accel.DeviceArray(ctx, (nbytes + GUARD,), np.uint8)
    ws.set(q, np.full(nbytes + GUARD, CANARY, np.uint8))
    check(L.kimg_fold_runs_mapped(dev[0].ptr, dev[1].ptr, dev[2].ptr, n, P, capacity, ws.ptr, nbytes,
                                  q.handle, fmap.ptr), 'kimg_fold_runs_mapped')
    q.finish()
    raw = ws.get(q)
    assert np.all(raw[nbytes:] == CANARY), 'written behind the workspace'
    raw = raw[:nbytes]
    hdr = dict(use_folded=int(raw[0:4].view(np.uint32)[0]), spans=int(raw[4:8].view(np.uint32)[0]),
               count=int(raw[8:16].view(np.int64)[0]), capacity=int(raw[40:48].view(np.int64)[0]))
    ptr = [int(x) for x in raw[16:40].view(np.uint64)]
    hdr['uv'], hdr['w_plane'] = ptr[0] - fmap.ptr, ptr[1] - fmap.ptr       # into the map
    hdr['vis'] = ptr[2] - ws.ptr                                            # into the workspace
    return hdr, raw


def compare_pass(ctx, q, uv, wp, vis, P, what):
    """The mapped pass against the planned one on one stream; checks the map's contents first."""
    n = len(uv)
    dev = (_dev(ctx, q, uv), _dev(ctx, q, wp), _dev(ctx, q, vis))
    plan, f, fmap, mraw = planned_map(ctx, q, dev[0], dev[1], n, P)
    check_map(mraw, uv, wp, f, what)
    H, cap = f['count'], n // 2
    a, araw = run_fold(ctx, q, dev, n, P, cap, plan)
    b, braw = run_mapped(ctx, q, dev, n, P, cap, fmap)
    for key in ('use_folded', 'spans', 'count', 'capacity'):
        assert a[key] == b[key], (what, key, a[key], b[key])
    assert a['count'] == H and a['use_folded'] == int(2 * H <= n), what
    body = HEADER_BYTES + COUNTS_BYTES
    (uv_at, uv_len), (w_at, w_len), (vis_at, vis_len) = a['sections']
    if not a['use_folded']:
        assert np.all(braw[body:] == CANARY), what
        return
    _, o_uv, o_w, _ = map_layout(n, H)
    assert (b['uv'], b['w_plane'], b['vis']) == (o_uv, o_w, vis_at), what
    # the sums, bit for bit, and nothing else: a mapped call writes no coordinates
    assert np.array_equal(araw[vis_at:vis_at + vis_len], braw[vis_at:vis_at + vis_len]), what
    assert np.all(braw[uv_at:uv_at + uv_len] == CANARY) and np.all(braw[w_at:w_at + w_len] == CANARY), what
    assert np.array_equal(a['uv'][:H], mraw[o_uv:o_uv + 8 * H].view(np.int16).reshape(H, 4)), what
    assert np.array_equal(a['w_plane'][:H], mraw[o_w:o_w + 2 * H].view(np.int16)), what
    sums = araw[vis_at:vis_at + 8 * P * H].view(np.float32)
    assert np.any(sums != np.round(sums)), what


@pytest.mark.parametrize('P', [1, 2, 3, 4])
def test_map_contents_and_mapped_fold_is_the_planned_fold(P):
    ctx, q = context_queue()
    rs = np.random.RandomState(160 + P)
    for n in SIZES:
        for kind in ('runs', 'exactly_half') if n >= 2 and n % 2 == 0 else ('runs',):
            uv, wp = fold_input(kind, n, rs)
            compare_pass(ctx, q, uv, wp, float_samples(rs, n, P), P, '%s n=%d P=%d' % (kind, n, P))


@pytest.mark.parametrize('P,n', SEVERAL)
def test_map_with_several_tiles_per_span(P, n):
    ctx, q = context_queue()
    rs = np.random.RandomState(5)
    uv, wp = fold_input('runs', n, rs)
    compare_pass(ctx, q, uv, wp, float_samples(rs, n, P), P, 'several tiles per span, P=%d' % P)


@pytest.mark.parametrize('P', [1, 3])
def test_mapped_fold_respects_the_capacity(P):
    """H above the capacity: refused, nothing written; at the capacity: the planned call's sums."""
    ctx, q = context_queue()
    rs = np.random.RandomState(9)
    n = 5 * TILE + 17
    uv, wp = fold_input('runs', n, rs)
    dev = (_dev(ctx, q, uv), _dev(ctx, q, wp), _dev(ctx, q, float_samples(rs, n, P)))
    plan, f, fmap, _ = planned_map(ctx, q, dev[0], dev[1], n, P)
    H = f['count']
    for capacity in (H - 1, 0):
        hdr, raw = run_mapped(ctx, q, dev, n, P, capacity, fmap)
        assert hdr['use_folded'] == 0 and hdr['count'] == H
        assert np.all(raw[HEADER_BYTES + COUNTS_BYTES:] == CANARY)
    a, araw = run_fold(ctx, q, dev, n, P, H, plan)
    hdr, raw = run_mapped(ctx, q, dev, n, P, H, fmap)
    assert a['use_folded'] == hdr['use_folded'] == 1
    vis_at, vis_len = a['sections'][2]
    assert np.array_equal(araw[vis_at:vis_at + vis_len], raw[vis_at:vis_at + vis_len])


# ---------------------------------------------------------------------------------------------
# through kimg_grid

def grid_mapped(call, fmap, bits=0):
    """Call.grid with kimg_grid_mapped -> (grid, header of the pre-pass)"""
    from katsdpimager_amd import grid
    from katsdpimager_amd._lib import check, lib
    c, q = call.case, call.q
    g = Padded(call.ctx, q, np.zeros((c.P, c.G, c.G), np.complex64), 3, 1, np.complex64(-1.5e7 + 3.25e6j))
    fill = np.full(call.nbytes + GUARD, CANARY, np.uint8)
    fill[:call.nbytes] = 0
    call.ws.set(q, fill)
    check(lib().kimg_grid_mapped(
        g.dev.ptr, g.row, g.pol, c.G, c.P, call.wg.dev.ptr, call.wg.row, call.wg.pol, call.uv.ptr,
        call.wp.ptr, call.vis.ptr, call.n, call.table.ptr, c.W, c.OV, c.K, call.ws.ptr, call.nbytes,
        grid.GRID_VARIANTS['mfma'] | c.cus << 8, grid.GRID_ARITH['fp32'] | bits, q.handle, fmap.ptr),
        'kimg_grid_mapped')
    q.finish()
    raw = call.ws.get(q)
    assert np.all(raw[call.nbytes:] == CANARY), 'written behind the workspace'
    raw = raw[call.own - 256:]
    return g.get(q), dict(use_folded=int(raw[0:4].view(np.uint32)[0]), count=int(raw[8:16].view(np.int64)[0]))


def map_of(call, n=None, P=None, plan_of=None):
    """A map of the call's stream (its first n records, the layout of P polarizations), from its own
    plan or from that of the call `plan_of`."""
    n, P = n or call.n, P or call.case.P
    plan, praw = make_plan(call.ctx, call.q, (plan_of or call).uv, (plan_of or call).wp, n, P)
    return make_map(call.ctx, call.q, call.uv, call.wp, n, P, plan, plan_fields(praw)['count'])


@pytest.mark.parametrize('case', GRID_CASES, ids=repr)
def test_mapped_grid_is_the_planned_grid(case):
    ctx, q = context_queue()
    inp, ok = _cut(*fold_stream(case), case.n)
    call = Call(ctx, q, case, inp)
    want, hdr = call.grid(0, call.plan())
    assert hdr['use_folded'] == 1
    fmap, raw = map_of(call)
    assert map_fields(raw)['valid'] == 1
    got, got_hdr = grid_mapped(call, fmap)
    assert got_hdr == hdr
    assert np.array_equal(_bits(got), _bits(want))
    _assert_exact(got, _truth(inp, ok), repr(case))
    got, got_hdr = grid_mapped(call, fmap, NO_FOLD)     # (ignored with the fold, like a plan)
    assert got_hdr == dict(use_folded=0, count=0) and np.array_equal(_bits(got), _bits(want))


def _refused(call, fmap, unfolded, what):
    got, hdr = grid_mapped(call, fmap)
    assert hdr['use_folded'] == 0, what
    assert np.array_equal(_bits(got), _bits(unfolded)), what


@pytest.mark.parametrize('P', [1, 3])
def test_refused_maps_never_change_the_grid(P):
    from katsdpimager_amd import accel
    ctx, q = context_queue()
    n = 5 * TILE + 17
    case = FoldCase('refused_p%d' % P, 28, 8, 4, P, n, 168)
    a = simple_stream('stale_a', 28, 8, 4, P, n, 168, [2, 3, 5, 9, 30])
    b = simple_stream('stale_b', 28, 8, 4, P, n, 168, [2, 4, 7, 40, 200])
    call_a, call_b = Call(ctx, q, case, a), Call(ctx, q, case, b)
    unfolded, _ = call_b.grid(NO_FOLD)
    _assert_exact(unfolded, _truth(b, np.ones(n, bool)), 'unfolded')
    fresh_map, fresh_raw = map_of(call_b)
    fresh, hdr = grid_mapped(call_b, fresh_map)
    assert hdr['use_folded'] == 1 and np.array_equal(_bits(fresh), _bits(unfolded))
    # maps of this stream for another length
    for m in (n - 1, 3 * TILE):
        fmap, raw = map_of(call_b, n=m)
        assert map_fields(raw)['valid'] == 1 and map_fields(raw)['num_vis'] == m
        _refused(call_b, fmap, unfolded, 'map for %d records' % m)
    # arbitrary bytes
    junk = accel.DeviceArray(ctx, (len(fresh_raw),), np.uint8)
    for byte in (0xFF, 0x00):
        junk.set(q, np.full(junk.shape, byte, np.uint8))
        _refused(call_b, junk, unfolded, 'map of %#x bytes' % byte)
    # stream A's plan on stream B: the spans count other heads than the plan's, the map is born invalid
    fmap, raw = map_of(call_b, plan_of=call_a)
    assert map_fields(raw)['magic'] == MAP_MAGIC and map_fields(raw)['valid'] == 0
    _refused(call_b, fmap, unfolded, "map from stream A's plan")
    # ... and a map that is in order except for that word
    raw = fresh_map.get(q)
    raw[40:44] = 0
    fresh_map.set(q, raw)
    _refused(call_b, fresh_map, unfolded, 'valid = 0')
    # a misaligned map is the one thing the host can see
    from katsdpimager_amd._lib import lib
    assert lib().kimg_fold_runs_mapped(call_b.uv.ptr, call_b.wp.ptr, call_b.vis.ptr, n, P, n // 2,
                                       call_b.ws.ptr, call_b.nbytes, q.handle, junk.ptr + 8) == -10001


def test_map_with_more_heads_than_the_capacity_is_refused():
    """A stream that does not fold: its map is valid, H is above the N / 2 records the call has room
    for, and the call grids the caller's stream."""
    ctx, q = context_queue()
    n = 5 * TILE + 17
    case = FoldCase('no_room', 28, 8, 4, 2, n, 168)
    inp = simple_stream(case.name, 28, 8, 4, 2, n, 168, [1, 1, 1, 2])
    call = Call(ctx, q, case, inp)
    fmap, raw = map_of(call)
    m = map_fields(raw)
    assert m['valid'] == 1 and m['count'] > n // 2
    unfolded, _ = call.grid(NO_FOLD)
    _assert_exact(unfolded, _truth(inp, np.ones(n, bool)), 'unfolded')
    _refused(call, fmap, unfolded, 'H above the capacity')


def test_map_of_another_polarization_layout_is_refused():
    """More than 512 tiles: two polarizations cut 601 spans of one tile, three 301 spans of two."""
    ctx, q = context_queue()
    n, G = 600 * TILE + 5, 1024
    case = FoldCase('layout', 28, 8, 4, 2, n, G, amp=1)
    inp = simple_stream(case.name, 28, 8, 4, 2, n, G, [2, 3, 4, 5], amp=1)
    assert _cover_bound(inp, 28, G) < EXACT
    call = Call(ctx, q, case, inp)
    unfolded, _ = call.grid(NO_FOLD)
    assert np.any(unfolded != 0)
    fmap, raw = map_of(call)
    fresh, hdr = grid_mapped(call, fmap)
    assert hdr['use_folded'] == 1 and np.array_equal(_bits(fresh), _bits(unfolded))
    fmap, raw = map_of(call, P=3)
    assert map_fields(raw)['valid'] == 1 and map_fields(raw)['spans'] == 301
    _refused(call, fmap, unfolded, 'map of the three-polarization layout')


@pytest.mark.parametrize('P', [1, 2, 3, 4])
def test_head_bits_cannot_move_a_write_out_of_bounds(P):
    """A valid header over head bits that are all set -- eight heads per thread where the counts
    promise fewer: the sums are wrong, and every one of them lies inside the capacity."""
    ctx, q = context_queue()
    rs = np.random.RandomState(21)
    n = 5 * TILE + 17
    uv, wp = fold_input('runs', n, rs)
    dev = (_dev(ctx, q, uv), _dev(ctx, q, wp), _dev(ctx, q, float_samples(rs, n, P)))
    plan, f, fmap, raw = planned_map(ctx, q, dev[0], dev[1], n, P)
    H = f['count']
    bits, o_uv, _, _ = map_layout(n, H)
    raw = fmap.get(q)
    raw[bits:o_uv] = 0xFF
    fmap.set(q, raw)
    for capacity in (n // 2, H):
        a, _ = run_fold(ctx, q, dev, n, P, capacity, plan)
        hdr, ws = run_mapped(ctx, q, dev, n, P, capacity, fmap)     # (asserts the guard behind the workspace)
        assert hdr['use_folded'] == 1 and hdr['count'] == H
        (uv_at, uv_len), (w_at, w_len), (vis_at, vis_len) = a['sections']
        assert vis_len == 8 * P * capacity and uv_len == 8 * capacity and w_len == 2 * capacity
        # behind the header and the counts nothing but the capacity's sums is touched
        assert np.all(ws[HEADER_BYTES + COUNTS_BYTES:vis_at] == CANARY)
        assert np.all(ws[vis_at + vis_len:] == CANARY)
    # and through the gridder: the call completes
    case = FoldCase('all_heads_p%d' % P, 28, 8, 4, P, n, 168)
    inp = simple_stream(case.name, 28, 8, 4, P, n, 168, [2, 3, 5, 9, 30])
    call = Call(ctx, q, case, inp)
    fmap, raw = map_of(call)
    H = map_fields(raw)['count']
    bits, o_uv, _, _ = map_layout(n, H)
    raw = fmap.get(q)
    raw[bits:o_uv] = 0xFF
    fmap.set(q, raw)
    got, hdr = grid_mapped(call, fmap)
    assert hdr == dict(use_folded=1, count=H) and np.all(np.isfinite(got))
