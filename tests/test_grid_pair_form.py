"""The float32 gridder's pair form (v_mfma_f32_16x16x4_f32, two visibilities per instruction, the
default) against the one-visibility form (v_mfma_f32_32x32x2_f32, ``arith='fp32_32x32'``).  Each
accumulator cell sees the same fmaf sequence in both, so the grids may differ only by the order of
the float atomics.  Run with ``-m gpu``."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from test_full_size import _setup, _grid_all        # noqa: E402

pytestmark = pytest.mark.gpu


def _compare(pixels, n, w_planes, P, K):
    ctx, q, obs, pair, wg = _setup(pixels, n, w_planes, P, K, variant='mfma', vis_block=n)
    _, _, _, single, _ = _setup(pixels, n, w_planes, P, K, variant='mfma', vis_block=n,
                                arith='fp32_32x32')
    single.bind(weights_grid=wg)
    got = _grid_all(ctx, q, obs, pair).clone()
    want = _grid_all(ctx, q, obs, single).clone()
    peak = float(want.abs().max())
    assert peak > 0
    assert float((got - want).abs().max()) <= 1e-6 * peak
    assert bool(((got != 0) == (want != 0)).all())


def test_pair_form_c2_geometry():
    """~1 M visibilities at C2 geometry (4096^2, 32 planes, K = 28, one polarization: the table in
    LDS, 12-wave blocks, doubled rows)."""
    _compare(4096, 1 << 20, 32, 1, 28)


def test_pair_form_tap_blocks_hbm_table_two_pols_odd():
    """K = 60 (2 x 2 tap blocks, two tables for the off-diagonal ones), 400 W planes (tables in HBM),
    two polarizations, an odd number of visibilities (the last one pairs with a zero partner)."""
    _compare(2048, (1 << 18) + 1, 400, 2, 60)
