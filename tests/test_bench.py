"""bench.py's plain run and --dump-outputs: what a plain run prints and writes on the GPU, and the
dump's format and size limit on the CPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import relerr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_float32_and_a_fixed_sample_over_the_limit(tmp_path):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    gen = torch.Generator().manual_seed(1)
    g = torch.complex(torch.randn((2, 300, 300), generator=gen), torch.randn((2, 300, 300), generator=gen))
    w = torch.rand((50, 7), generator=gen)
    bench.dump_outputs(str(tmp_path / 'all'), {'grid': g, 'w': w})
    grid = np.load(str(tmp_path / 'all' / 'grid.npy'))
    assert grid.dtype == np.float32 and grid.shape == (2, 300, 300, 2)
    np.testing.assert_array_equal(grid[..., 0], g.real.numpy())
    np.testing.assert_array_equal(grid[..., 1], g.imag.numpy())
    np.testing.assert_array_equal(np.load(str(tmp_path / 'all' / 'w.npy')), w.numpy())
    # over the limit: every array cut to the same seeded sample, in flat index order, every time
    limit = 100_000
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), {'grid': g, 'w': w}, limit=limit)
    a, b = (np.load(str(tmp_path / d / 'grid.npy')) for d in ('a', 'b'))
    wa = np.load(str(tmp_path / 'a' / 'w.npy'))
    assert a.dtype == np.float32 and wa.dtype == np.float32
    assert a.nbytes + wa.nbytes <= limit
    np.testing.assert_array_equal(a, b)
    n = 2 * 300 * 300
    total = n * 8 + w.numel() * 4
    idx = np.unique(np.random.RandomState(0).randint(0, n, n * limit // total))
    np.testing.assert_array_equal(a, grid.reshape(-1, 2)[idx])


@pytest.mark.gpu
def test_plain_run_times_the_headline_and_dumps_its_last_step(tmp_path):
    """A plain `bench.py` (no --full): the headline alone, `--steps` timed steps, and
    --dump-outputs writes the grid of the last one -- the same grid after 1 step as after a
    warm-up and 3 (every step clears the grid; the inputs are seeded)."""
    grids = {}
    for steps, warmup in ((1, 0), (3, 1)):
        d = tmp_path / str(steps)
        out = subprocess.run(
            [sys.executable, os.path.join(ROOT, 'bench.py'), '--vis', '2000000', '--steps', str(steps),
             '--warmup', str(warmup), '--dump-outputs', str(d)],
            capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [x for x in out.stdout.splitlines() if x.startswith('{')]
        assert len(lines) == 1
        line = json.loads(lines[0])
        assert line['steps'] == steps and line['warmup'] == warmup and line['ms_per_step'] > 0
        assert line['unit'] == 'Mvis/s' and line['higher_is_better'] is True and line['dtype'] == 'f32'
        assert not {'split_fp16', 'cpu_baseline', 'secondary', 'major_cycle_loop'} & set(line)
        G = line['config']['grid_size']
        grid = np.load(str(d / 'grid.npy'))
        assert grid.dtype == np.float32 and grid.shape == (1, G, G, 2)
        grids[steps] = grid
    assert np.abs(grids[1]).max() > 0
    assert relerr(grids[3], grids[1]) < 1e-5
