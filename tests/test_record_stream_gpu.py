"""The units that re-order and compact the record stream (csrc/store.hip, preprocess.hip,
grid_binned.hip, grid_fold.hip) at the sizes where what they share (csrc/kimg_record_stream.h) can go
wrong: one record, the edges of a 256-thread block, the two sides of STORE_MAX_RUN, a sort whose
largest key is the sentinel, and a workspace whose pieces are tiny.  Every comparison is bit for bit,
against the same references as the large cases of test_preprocess_gpu.py and test_exact_gridding.py,
whose helpers are imported and not copied."""
import numpy as np
import pytest

from helpers import context_queue
from oracle import kimg_oracle as orc
import test_exact_gridding as te
import test_preprocess_gpu as tp

pytestmark = pytest.mark.gpu

KIMG_EWORKSPACE = -10003
SIZES = (1, 2, 255, 256, 257, 4095, 4096, 4097)     # (the last three straddle STORE_MAX_RUN)


# ---- kimg_store_reorder ------------------------------------------------------------------------------
def _store_reorder(ctx, q, arrays, P, K, OV, W, merge, short_first=False):
    from katsdpimager_amd import accel
    from katsdpimager_amd._lib import lib, check
    L = lib()
    n = len(arrays[0])
    d = [te._dev(ctx, q, a) for a in arrays]
    o = [accel.DeviceArray(ctx, a.shape, a.dtype) for a in arrays]
    count = accel.DeviceArray(ctx, (1,), np.int64)
    ws_bytes = int(L.kimg_store_reorder_workspace_bytes(n))
    assert ws_bytes > 0 and ws_bytes % 256 == 0
    ws = accel.DeviceArray(ctx, (ws_bytes,), np.uint8)

    def call(nbytes):
        return L.kimg_store_reorder(P, n, K, OV, W, int(merge), d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr,
                                    o[0].ptr, o[1].ptr, o[2].ptr, o[3].ptr, count.ptr, ws.ptr, nbytes,
                                    q.handle)
    if short_first:
        assert call(ws_bytes - 1) == KIMG_EWORKSPACE
    check(call(ws_bytes), 'kimg_store_reorder')
    m = int(count.get(q)[0])
    return [a.get(q)[:m] for a in o]


def _store_stream(rs, n, P, W, OV, equal):
    """n records drawn from n // 3 + 1 places spread over several strips (so that a merge finds
    runs), or all at one place."""
    places = 1 if equal else n // 3 + 1
    at = np.concatenate([rs.randint(-40, 41, (places, 2)), rs.randint(0, OV, (places, 2)),
                         rs.randint(0, W, (places, 1))], axis=1).astype(np.int16)
    rec = at[rs.randint(0, places, n)]
    weights = rs.uniform(0.5, 2.0, (n, P)).astype(np.float32)
    vis = (rs.standard_normal((n, P)) + 1j * rs.standard_normal((n, P))).astype(np.complex64)
    return np.ascontiguousarray(rec[:, :4]), np.ascontiguousarray(rec[:, 4]), weights, vis


@pytest.mark.parametrize('equal', [False, True], ids=['random', 'equal'])
@pytest.mark.parametrize('n', SIZES)
def test_store_reorder_at_block_and_run_edges(n, equal):
    """kimg_store_reorder against oracle.store_reorder, every output array bit for bit, with merge off
    and on, P = 1 and 4, K = 28 (strips of 5 columns) and 45 (two tap blocks, strips of 10); at n = 1
    also the refusal of a workspace one byte short."""
    ctx, q = context_queue()
    W, OV = 3, 4
    for P in (1, 4):
        for K in (28, 45):
            rs = np.random.RandomState(n * 11 + P * 3 + K)
            arrays = _store_stream(rs, n, P, W, OV, equal)
            for merge in (False, True):
                got = _store_reorder(ctx, q, arrays, P, K, OV, W, merge, short_first=(n == 1))
                want = orc.store_reorder(*arrays, K, OV, W, merge)
                what = 'n=%d P=%d K=%d merge=%s' % (n, P, K, merge)
                if not merge:
                    assert len(want[0]) == n, what
                elif equal:
                    assert len(want[0]) == -(-n // orc.STORE_MAX_RUN), what
                elif n > 2:
                    assert len(want[0]) < n, what
                assert len(got[0]) == len(want[0]), what
                for g, w_ in zip(got, want):
                    np.testing.assert_array_equal(g.view(np.uint8),
                                                  np.ascontiguousarray(w_).view(np.uint8), what)


# ---- the device collector ----------------------------------------------------------------------------
@pytest.mark.parametrize('w_slices', [1, 3])
@pytest.mark.parametrize('buffer_size', [1, 256, 257])
@pytest.mark.parametrize('P,Q', [(1, 2), (3, 4)])
def test_collector_at_block_edges(P, Q, buffer_size, w_slices):
    """The device collector against oracle.VisibilityCollector (tp._compare: indices and float sums bit
    for bit) with buffers of one record, of one 256-thread block and of one record more, one w-slice
    and three (the sort by slice and the gather after it), a conversion off the diagonal of the
    (P, Q) dispatch, and one buffer whose records are all flagged."""
    rng = np.random.default_rng(buffer_size * 10 + P + w_slices)
    configs = [dict(max_w=320.0, w_slices=w_slices, w_planes=16, oversample=8, cell_size=1.7)]
    stokes = (rng.normal(size=(P, Q)) + 1j * rng.normal(size=(P, Q))).astype(np.complex64)
    stokes[0, 0] = 0                                    # (the MulZ zero rule)
    n = 3 * 257 + 5
    uvw, weights, vis = tp._random_batch(rng, 1, n, Q)
    weights[:, buffer_size:2 * buffer_size, :] = 0      # the second buffer: nothing valid
    batch = (uvw, weights, vis, None, None, stokes, None)
    coll = tp._collect_device(configs, P, buffer_size, [batch])
    ref = orc.VisibilityCollector(configs, P, buffer_size)
    ref.add(*batch)
    assert 0 < ref.num_output < ref.num_input
    tp._compare(coll, ref, configs, True, P)


# ---- the tile-binned variants -------------------------------------------------------------------------
def _binned_case(n, outside, degrid):
    """An integer-table case of test_exact_gridding.py cut down to n records; with `outside`, the
    middle one lies one cell past the grid's edge along u: it takes bin_key_kernel's last_key, the
    largest key of the sort, and contributes nothing.  Returns (case, inputs, rows inside)."""
    case = te.Case('record_stream_%d' % n, 8, 4, 4, 1 + n % 2, 'random', n, seed=77 + n)
    inp = te._inputs(case, degrid=degrid)
    inside = np.ones(n, bool)
    if outside:
        inp['uv'][n // 2, 0] = case.G // 2              # u + G / 2 = G
        inside[n // 2] = False
    return case, inp, inside


@pytest.mark.parametrize('outside', [False, True], ids=['inside', 'one_outside'])
@pytest.mark.parametrize('n', [1, 256, 257])
def test_binned_grid_exact_at_block_edges(n, outside):
    ctx, q = context_queue()
    case, inp, inside = _binned_case(n, outside, False)
    want = np.zeros((case.P, case.G, case.G), np.complex128)
    if inside.any():
        canvas, bound = te.grid_truth(inp['kern'], inp['uv'][inside], inp['w_plane'][inside],
                                      inp['vis'][inside], inp['wg'])
        assert bound.max() < te.EXACT
        want = te._crop(canvas)
    for arith in te.GRID_FORMS:
        te._assert_exact(te.run_grid(ctx, q, case, inp, 'binned', arith), want, 'binned/%s' % arith)


@pytest.mark.parametrize('outside', [False, True], ids=['inside', 'one_outside'])
@pytest.mark.parametrize('n', [1, 256, 257])
def test_binned_degrid_exact_at_block_edges(n, outside):
    """(the record outside the grid gets no prediction: its visibility comes back as it went in)"""
    ctx, q = context_queue()
    case, inp, inside = _binned_case(n, outside, True)
    want = np.asarray(inp['vis'], np.complex128).copy()
    if inside.any():
        want[inside], bound = te.degrid_truth(inp['kern'], inp['uv'][inside], inp['w_plane'][inside],
                                              inp['weights'][inside], inp['vis'][inside], inp['grid'])
        assert bound.max() < te.EXACT
    for arith in te.DEGRID_FORMS:
        te._assert_exact(te.run_degrid(ctx, q, case, inp, 'binned', arith), want, 'binned/%s' % arith)


# ---- workspace sizes ----------------------------------------------------------------------------------
@pytest.mark.parametrize('P', [1, 4])
def test_workspace_sizes(P):
    """Every size query of the family: a multiple of 256, never smaller for more records, and the
    unit's refusal at n = 0 and n = 2^31.  (The byte counts themselves are not pinned: the sort's and
    the scans' temporary storage is the installed rocPRIM's.)"""
    from katsdpimager_amd._lib import lib
    L = lib()
    W, OV, K = 4, 4, 28
    queries = {
        'store_reorder': lambda n: L.kimg_store_reorder_workspace_bytes(n),
        'preprocess': lambda n: L.kimg_preprocess_workspace_bytes(n, P),
        'grid_binned': lambda n: L.kimg_grid_binned_workspace_bytes(n, P, W, OV, K),
        'degrid_binned': lambda n: L.kimg_degrid_binned_workspace_bytes(n, P, W, OV, K),
        'fold_runs': lambda n: L.kimg_fold_runs_workspace_bytes(P, n),
    }
    for name, query in queries.items():
        sizes = [int(query(n)) for n in SIZES]
        assert all(s > 0 and s % 256 == 0 for s in sizes), (name, sizes)
        assert sizes == sorted(sizes), (name, sizes)
        if name == 'fold_runs':
            # a capacity of no records is a valid one (the header and the spans' counts), and 2^31
            # records are no limit of the pre-pass; what it refuses is a negative capacity
            assert int(query(0)) == 256 + 4096 <= sizes[0]
            assert int(query(1 << 31)) % 256 == 0 and int(query(1 << 31)) > sizes[-1]
            assert int(query(-1)) == 0 and int(L.kimg_fold_runs_workspace_bytes(5, 1)) == 0
        else:
            assert int(query(0)) == 0 and int(query(1 << 31)) == 0, name
