"""Fold maps without a GPU: the C ABI's declarations and refusals, and the rules by which the Python
side keeps and drops a map -- those of the plan it belongs to (test_fold_plan_host.py)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from katsdpimager_amd import _lib, grid, preprocess        # noqa: E402
from test_fold_plan_host import Buf, Queue, Store, gridder        # noqa: E402

KIMG_EINVAL, KIMG_EUNSUPPORTED, KIMG_EWORKSPACE = -10001, -10002, -10003
NAMES = ('kimg_fold_map_bytes', 'kimg_fold_map', 'kimg_fold_runs_mapped', 'kimg_grid_mapped')
MAP = 0xA000


def plan_of(n, heads, P=1, fmap=MAP):
    return grid.FoldPlan(Buf(0x9000), heads, n, P, Buf(fmap) if fmap else None)


def test_symbols_declared_exported_and_prototyped():
    header = open(os.path.join(ROOT, 'include', 'kimg.h')).read()
    exported = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True,
                              text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r'\b%s\s*\(' % name, header), name
        assert name in _lib.PROTOTYPES and re.search(r' T %s\b' % name, exported), name
    assert _lib.PROTOTYPES['kimg_grid_mapped'][1] == _lib.PROTOTYPES['kimg_grid'][1] + [_lib.P]
    assert _lib.PROTOTYPES['kimg_grid_mapped'] == _lib.PROTOTYPES['kimg_grid_planned']
    assert _lib.PROTOTYPES['kimg_fold_runs_mapped'][1] == _lib.PROTOTYPES['kimg_fold_runs'][1] + [_lib.P]
    assert _lib.lib().kimg_version() == _lib.VERSION == 5


def test_map_bytes():
    """4160 bytes of header and counts, a byte per 8 records padded to 16, 10 bytes per head in
    eights: ``num_vis / 8 + 10 H`` and every section 16-byte aligned."""
    L = _lib.lib()
    assert L.kimg_fold_map_bytes(1, 1, 0) == 4160 + 16
    assert L.kimg_fold_map_bytes(128, 4, 1) == 4160 + 16 + 80
    assert L.kimg_fold_map_bytes(129, 2, 8) == 4160 + 32 + 80
    assert L.kimg_fold_map_bytes(129, 2, 9) == 4160 + 32 + 160
    n, H = 50_000_000, 7_080_000
    assert L.kimg_fold_map_bytes(n, 1, H) == 4160 + n // 8 + 10 * H
    for bad in ((0, 1, 0), (8, 0, 0), (8, 5, 0), (8, 1, -1)):
        assert L.kimg_fold_map_bytes(*bad) == 0


def test_mapped_calls_refuse_what_the_planned_ones_refuse():
    """Before any device work: null and misaligned pointers, a short buffer, the planned call's checks."""
    L = _lib.lib()
    buf = (ctypes.c_char * 16384)()
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    W = 64

    def call(row=W, wg_row=W, arith=0, fmap=p):
        return L.kimg_grid_mapped(p, row, W * W, W, 1, p, wg_row, W * W, p, p, p, 4, p, 1, 1, 7, p, 1 << 20,
                                  0, arith, None, fmap)
    assert call(row=63) == KIMG_EINVAL
    assert call(wg_row=63) == KIMG_EINVAL
    assert call(arith=0x400 | 0x800) == KIMG_EINVAL
    assert call(fmap=p + 8) == KIMG_EINVAL
    assert L.kimg_fold_runs_mapped(p, p, p, 4, 1, 2, p, 1 << 20, None, p + 4) == KIMG_EINVAL
    assert L.kimg_fold_runs_mapped(p, p, p, 0, 1, 2, p, 1 << 20, None, p) == KIMG_EINVAL
    nbytes = L.kimg_fold_map_bytes(4, 1, 2)
    assert L.kimg_fold_map(p, p, 0, 1, p, p, nbytes, None) == KIMG_EINVAL
    assert L.kimg_fold_map(p, p + 2, 4, 1, p, p, nbytes, None) == KIMG_EINVAL
    assert L.kimg_fold_map(p, p, 4, 1, None, p, nbytes, None) == KIMG_EINVAL
    assert L.kimg_fold_map(p, p, 4, 1, p, None, nbytes, None) == KIMG_EINVAL
    assert L.kimg_fold_map(p, p, 4, 1, p + 8, p, nbytes, None) == KIMG_EINVAL
    assert L.kimg_fold_map(p, p, 4, 1, p, p + 8, nbytes, None) == KIMG_EINVAL
    assert L.kimg_fold_map(p, p, 4, 1, p, p, L.kimg_fold_map_bytes(4, 1, 0) - 1, None) == KIMG_EWORKSPACE
    assert L.kimg_fold_map(p, p, 4, 5, p, p, nbytes, None) == KIMG_EUNSUPPORTED


def test_a_map_is_used_and_fold_map_false_takes_the_planned_call():
    n = 9 << 20
    g = gridder(n)
    g.set_fold_plan(plan_of(n, n // 2))
    assert g._fold_call() == ('kimg_grid_mapped', 0, (MAP,))
    g.template.fold_map = False
    assert g._fold_call() == ('kimg_grid_planned', 0, (0x9000,))
    g.template.fold_map = True
    g.set_fold_plan(plan_of(n, n // 2, fmap=None))          # a plan without a map: as before
    assert g._fold_call() == ('kimg_grid_planned', 0, (0x9000,))
    g.set_fold_plan(plan_of(n, n // 2 + 1))                 # does not fold: the map is not looked at
    assert g._fold_call() == ('kimg_grid', grid.GRID_ARITH_NO_PREFOLD, ())
    off = gridder(n, fold_runs=False)
    off.set_fold_plan(plan_of(n, 1))
    assert off._fold_call() == ('kimg_grid', grid.GRID_ARITH_NO_FOLD, ())


def test_the_tuning_key():
    assert grid._tuning({'fold_map': False}) == (0, 0, True)
    with pytest.raises(ValueError):
        grid._tuning({'fold_map': 'no'})

    class Fixed:
        real_dtype = 'float32'
    for tuning, want in ((None, True), ({}, True), ({'fold_map': True}, True), ({'fold_map': False}, False)):
        assert grid.GridderTemplate(None, Fixed, None, tuning).fold_map is want


def test_rebinding_coordinates_or_another_length_drops_the_map():
    n = 5000
    for drop in ('uv', 'w_plane', 'num_vis', 'num_vis_same', 'vis', 'slot'):
        g = gridder(n)
        g.set_fold_plan(plan_of(n, 100))
        assert g._fold_call() == ('kimg_grid_mapped', 0, (MAP,))
        if drop == 'num_vis':
            g.num_vis = n - 1
        elif drop == 'num_vis_same':
            g.num_vis = n
        elif drop == 'slot':            # (the way a compound slot of an OperationSequence binds)
            g.slots['uv'].bind(Buf(0x7000))
        else:
            g.bind(**{drop: Buf(0x8000)})
        kept = drop in ('vis', 'num_vis_same')
        assert g._fold_call() == (('kimg_grid_mapped', 0, (MAP,)) if kept else ('kimg_grid', 0, ())), drop
    g = gridder(n)
    g.set_fold_plan(plan_of(n, 100))
    g.num_vis = n - 1
    g.num_vis = n                       # back at the old length: the map is gone all the same
    assert g._fold_call() == ('kimg_grid', 0, ())
    for wrong in (plan_of(n - 1, 100), plan_of(n, 100, P=2)):   # a map of another stream's plan
        g.set_fold_plan(wrong)
        assert g._fold_call() == ('kimg_grid', 0, ())


def test_a_copied_hint_carries_no_map():
    n = 5000
    a, b = gridder(n), gridder(n, hint=None)
    a.set_fold_plan(plan_of(n, 100))
    b.locality_hint = a.locality_hint
    assert b.locality_hint is True and b.fold_plan is None and b._fold_call() == ('kimg_grid', 0, ())


def test_measure_fold_plan_makes_a_map_only_for_a_stream_that_folds(monkeypatch):
    n, made = 4096, []

    class Array(Buf):
        def __init__(self, context, shape, dtype, queue=None):
            super().__init__(0x10000 * (len(made) + 1), shape)
            made.append(self)

        def get(self, queue):
            import numpy as np
            raw = np.zeros(self.shape, np.uint8)
            raw[24:32].view(np.int64)[0] = heads
            return raw

    class Lib:
        kimg_fold_plan_bytes = staticmethod(lambda: 4160)
        kimg_fold_map_bytes = staticmethod(lambda n, P, H: 5000 + H)

        def __init__(self):
            self.calls = []

        def kimg_fold_plan(self, *args):
            self.calls.append(('plan',) + args)
            return 0

        def kimg_fold_map(self, *args):
            self.calls.append(('map',) + args)
            return 0

    class Q(Queue):
        context, handle = None, 0x77
    monkeypatch.setattr(grid.accel, 'DeviceArray', Array)
    for heads, folds in ((n // 2, True), (n // 2 + 1, False)):
        L = Lib()
        monkeypatch.setattr(grid, 'lib', lambda: L)
        del made[:]
        fp = grid.measure_fold_plan(Q(), Buf(0x1000), Buf(0x2000), n, 2)
        assert (fp.heads, fp.num_vis, fp.polarizations, fp.foldable) == (heads, n, 2, folds)
        assert [c[0] for c in L.calls] == (['plan', 'map'] if folds else ['plan'])
        if folds:
            assert fp.map is made[1] and made[1].shape == (5000 + heads,)
            assert L.calls[1] == ('map', 0x1000, 0x2000, n, 2, made[0].ptr, made[1].ptr, 5000 + heads, 0x77)
        else:
            assert fp.map is None


def test_the_store_drops_a_slices_map_with_its_records(monkeypatch):
    s = Store()
    s.append(s._allocate(10), 0, 10)
    s.fold_plan = plan_of(10, 3)
    s.ensure_slack(1000)                # reallocated, the same bytes: the map still holds
    assert s.fold_plan is not None and s.fold_plan.map is not None
    s.append(s._allocate(5), 0, 5)
    assert s.fold_plan is None
    s.fold_plan = plan_of(15, 3)
    monkeypatch.setattr(preprocess, 'reorder_device_arrays', lambda *a, **k: (s._allocate(15), 15))
    s.reorder(28, 8, 4, False)
    assert s.fold_plan is None
    s.fold_plan = plan_of(15, 3)
    c = object.__new__(preprocess.VisibilityCollectorDevice)
    c._closed, c.reorder, c._stores = False, False, [[s]]
    c.close()
    assert s.fold_plan is None
