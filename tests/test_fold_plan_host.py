"""Fold plans without a GPU: the C ABI's declarations and refusals, and the rules by which the Python
side keeps, hands on and drops a plan (grid.Gridder, preprocess._SliceStore, the reader's chunks)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from katsdpimager_amd import _lib, grid, preprocess        # noqa: E402

KIMG_EINVAL = -10001
NAMES = ('kimg_fold_plan_bytes', 'kimg_fold_plan', 'kimg_fold_runs_planned', 'kimg_grid_planned')


def test_symbols_declared_exported_and_prototyped():
    header = open(os.path.join(ROOT, 'include', 'kimg.h')).read()
    exported = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True,
                              text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r'\b%s\s*\(' % name, header), name
        assert name in _lib.PROTOTYPES and re.search(r' T %s\b' % name, exported), name
    assert _lib.PROTOTYPES['kimg_grid_planned'][1] == _lib.PROTOTYPES['kimg_grid'][1] + [_lib.P]
    assert _lib.PROTOTYPES['kimg_fold_runs_planned'][1] == _lib.PROTOTYPES['kimg_fold_runs'][1] + [_lib.P]
    assert '#define KIMG_ARITH_NO_PREFOLD 0x800' in header and grid.GRID_ARITH_NO_PREFOLD == 0x800
    assert _lib.lib().kimg_version() == _lib.VERSION == 5
    assert _lib.lib().kimg_fold_plan_bytes() == 64 + 4 * 1024


def test_planned_calls_refuse_what_the_unplanned_ones_refuse():
    """Before any device work: strides below the width, PREFOLD with NO_PREFOLD, a misaligned plan."""
    L = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    W = 64

    def call(row=W, wg_row=W, arith=0, plan=p):
        return L.kimg_grid_planned(p, row, W * W, W, 1, p, wg_row, W * W, p, p, p, 4, p, 1, 1, 7, p, 1 << 20,
                                   0, arith, None, plan)
    assert call(row=63) == KIMG_EINVAL
    assert call(wg_row=63) == KIMG_EINVAL
    assert call(arith=0x400 | 0x800) == KIMG_EINVAL
    assert call(arith=0x200) == KIMG_EINVAL
    assert call(plan=p + 8) == KIMG_EINVAL
    assert L.kimg_fold_runs_planned(p, p, p, 4, 1, 2, p, 1 << 20, None, p + 4) == KIMG_EINVAL
    assert L.kimg_fold_runs_planned(p, p, p, 0, 1, 2, p, 1 << 20, None, p) == KIMG_EINVAL
    assert L.kimg_fold_plan(p, p, 0, 1, p, None) == KIMG_EINVAL
    assert L.kimg_fold_plan(p, p + 2, 4, 1, p, None) == KIMG_EINVAL
    assert L.kimg_fold_plan(p, p, 4, 1, None, None) == KIMG_EINVAL


# ---------------------------------------------------------------------------------------------
# grid.Gridder

class Buf:
    def __init__(self, ptr, shape=()):
        self.ptr, self.shape = ptr, shape

    def used_on(self, queue):
        pass


class Slot:
    def __init__(self, buffer=None, shape=()):
        self.buffer, self.shape = buffer, shape

    def bind(self, buffer):
        self.buffer = buffer


class Template:
    def __init__(self, variant='auto', fold_runs=True):
        self.variant, self.fold_runs, self.arith = grid.GRID_VARIANTS[variant], fold_runs, 0


def gridder(n=9 << 20, variant='auto', fold_runs=True, hint=True, P=1):
    """A Gridder with what the fold-plan rules look at, and nothing that needs a device."""
    g = object.__new__(grid.Gridder)
    g.command_queue = None
    g.template = Template(variant, fold_runs)
    g.slots = {'uv': Slot(Buf(0x1000)), 'w_plane': Slot(Buf(0x2000)), 'vis': Slot(Buf(0x3000)),
               'grid': Slot(Buf(0x4000), (P, 64, 64))}
    g.max_vis = 16 << 20
    g._num_vis = n
    g._f64 = False
    g._binned_bytes = 1
    g._workspace_bytes = 1 << 60        # (never grown here)
    g.locality_hint = hint

    class Table:
        padded_data = Buf(0x5000, (4, 8, 28))
    g.convolve_kernel = Table
    return g


def plan_of(n, heads, P=1):
    return grid.FoldPlan(Buf(0x9000), heads, n, P)


def test_a_plan_is_used_and_says_whether_the_stream_folds():
    n = 9 << 20
    g = gridder(n)
    assert g._fold_call() == ('kimg_grid', 0, ())               # no measurement: as before
    g.set_fold_plan(plan_of(n, n // 2))
    assert g.fold_plan is not None and g._fold_call() == ('kimg_grid_planned', 0, (0x9000,))
    # not foldable: the pre-pass is skipped, also above the 8 Mi records from which a call takes it
    assert n >= 8 << 20
    g.set_fold_plan(plan_of(n, n // 2 + 1))
    assert g._fold_call() == ('kimg_grid', grid.GRID_ARITH_NO_PREFOLD, ())
    g.set_fold_plan(None)
    assert g.fold_plan is None and g._fold_call() == ('kimg_grid', 0, ())
    off = gridder(n, fold_runs=False)
    off.set_fold_plan(plan_of(n, 1))
    assert off.fold_plan is None and off._fold_call() == ('kimg_grid', grid.GRID_ARITH_NO_FOLD, ())


def test_rebinding_coordinates_or_another_length_drops_the_plan():
    n = 5000
    for drop in ('uv', 'w_plane', 'num_vis', 'num_vis_same', 'vis', 'slot'):
        g = gridder(n)
        g.set_fold_plan(plan_of(n, 100))
        assert g.fold_plan is not None
        if drop == 'num_vis':
            g.num_vis = n - 1
        elif drop == 'num_vis_same':
            g.num_vis = n
        elif drop == 'slot':            # (the way a compound slot of an OperationSequence binds)
            g.slots['uv'].bind(Buf(0x7000))
        else:
            g.bind(**{drop: Buf(0x8000)})
        kept = drop in ('vis', 'num_vis_same')
        assert (g.fold_plan is not None) == kept, drop
        assert g._fold_call()[0] == ('kimg_grid_planned' if kept else 'kimg_grid'), drop
    g = gridder(n)
    g.set_fold_plan(plan_of(n, 100))
    g.num_vis = n - 1
    g.num_vis = n                       # back at the old length: the plan is gone all the same
    assert g.fold_plan is None
    with pytest.raises(ValueError):
        g.num_vis = g.max_vis + 1


def test_a_copied_hint_carries_no_plan():
    n = 5000
    a, b = gridder(n), gridder(n, hint=None)
    a.set_fold_plan(plan_of(n, 100))
    b.locality_hint = a.locality_hint
    assert b.locality_hint is True and b.fold_plan is None and b._fold_call() == ('kimg_grid', 0, ())
    assert a.locality_hint is True and not isinstance(a.locality_hint, grid.FoldPlan)


def test_plans_that_cannot_be_the_streams_are_ignored():
    n = 5000
    for kwargs, plan in ((dict(), plan_of(n - 1, 100)), (dict(P=2), plan_of(n, 100, P=1)),
                         (dict(variant='generic'), plan_of(n, 100)), (dict(variant='binned'), plan_of(n, 100)),
                         (dict(hint=None), plan_of(n, 100)), (dict(hint=False), plan_of(n, 100))):
        g = gridder(n, **kwargs)
        g.set_fold_plan(plan)
        assert g.fold_plan is None, kwargs
    g = gridder(n, variant='mfma', hint=None)
    g.set_fold_plan(plan_of(n, 100))
    assert g.fold_plan is not None
    for name in ('uv', 'w_plane', 'vis'):       # (the pre-pass reads 16 bytes at a time)
        g = gridder(n)
        g.slots[name].buffer = Buf(0x1008)
        g.set_fold_plan(plan_of(n, 100))
        assert g.fold_plan is None, name
    g = gridder(n)
    g._f64 = True
    g.set_fold_plan(plan_of(n, 100))
    assert g.fold_plan is None


# ---------------------------------------------------------------------------------------------
# the resident store

class Array(Buf):
    def copy_region(self, *args):
        pass


class Queue:
    def finish(self):
        pass


class Store(preprocess._SliceStore):
    def __init__(self):
        super().__init__(None, Queue(), 1, 0)

    def _allocate(self, rows):
        return {name: Array(0x100 * (i + 1) + rows) for i, name in enumerate(('uv', 'w_plane', 'weights', 'vis'))}

    def view(self, start, rows):
        return dict(self.arrays)


def test_the_store_drops_a_slices_plan_when_its_records_change(monkeypatch):
    s = Store()
    s.append(s._allocate(10), 0, 10)
    s.fold_plan = plan_of(10, 3)
    before = s.arrays
    s.ensure_slack(1000)                # reallocated, same records
    assert s.arrays is not before and s.fold_plan is not None
    s.append(s._allocate(5), 0, 5)
    assert s.fold_plan is None
    s.fold_plan = plan_of(15, 3)
    monkeypatch.setattr(preprocess, 'reorder_device_arrays', lambda *a, **k: (s._allocate(15), 15))
    s.reorder(28, 8, 4, False)
    assert s.ordered and s.fold_plan is None
    s.fold_plan = plan_of(15, 3)
    c = object.__new__(preprocess.VisibilityCollectorDevice)
    c._closed, c.reorder, c._stores = False, False, [[s]]
    c.close()
    assert s.fold_plan is None


def test_a_chunk_carries_the_plan_only_when_it_is_the_whole_slice(monkeypatch):
    s = Store()
    s.append(s._allocate(100), 0, 100)
    s.ordered = True

    class Fixed:
        kernel_width = 28

    class GP:
        fixed = Fixed

    class Collector:
        buffer_size, merge, queue, grid_parameters = 40, False, None, [GP]
    r = object.__new__(preprocess.VisibilityReaderDevice)
    r.collector, r._stores, r._locality_cache = Collector, [[s]], {}
    made = []

    def measure(queue, uv, w_plane, n, P):
        made.append((uv.ptr, w_plane.ptr, n, P))
        return plan_of(n, 7, P)
    monkeypatch.setattr(grid, 'measure_fold_plan', measure)
    assert [c.fold_plan for c in r.iter_slice_device(0, 0)] == [None] * 3 and not made
    for _ in range(2):                  # measured once
        chunks = list(r.iter_slice_device(0, 0, block_size=100))
        assert len(chunks) == 1 and chunks[0].fold_plan is s.fold_plan and chunks[0].locality is True
        assert chunks[0].fold_plan.num_vis == chunks[0].num_vis == 100
    assert made == [(s.arrays['uv'].ptr, s.arrays['w_plane'].ptr, 100, 1)]
    Collector.merge = True              # a merged slice has no runs to fold
    assert [c.fold_plan for c in r.iter_slice_device(0, 0, block_size=100)] == [None]
