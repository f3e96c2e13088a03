"""The cache of captured minor-cycle graphs (csrc/kimg_graph_cache.h) past its capacity: 32 argument
sets.  Forty PSF patch sizes on one set of buffers are forty argument sets, and every call of 64
cycles asks for a graph (64 >= KIMG_GRAPH_CYCLES / 2), so at least eight of the calls have to evict
an entry or fall back to plain launches.  Whichever it was, a call whose entry is gone gives what
the per-call form (no graphs) gives, bit for bit."""
import functools

import pytest

from test_clean_mask import make_clean, problem, run, same_run, start

gpu = pytest.mark.gpu

P, MODE = 1, 0
CYCLES = 64
# 15 widths x 3 heights, the first 40: all of 3 x 3 lattice blocks (the one-launch form runs), all
# within the 256 x 256 PSF
PATCHES = [(P, h, w) for h in (33, 39, 47) for w in range(33, 48)][:40]


@functools.lru_cache(maxsize=None)
def per_call():
    """The problem and CYCLES cycles of the first patch size in the per-call form."""
    psf, dirty = problem(MODE, P)
    fn, q = make_clean(P, MODE, dirty, psf, 'per_call')
    start(fn, q, dirty, None)
    return psf, dirty, run(fn, q, 'per_call', PATCHES[0], 0.0, CYCLES)


@gpu
@pytest.mark.parametrize('form', ['two_launch', 'one_launch'])
def test_more_argument_sets_than_slots(form):
    assert len(set(PATCHES)) == 40 > 32
    psf, dirty, want = per_call()
    assert len(want[0]) == CYCLES
    fn, q = make_clean(P, MODE, dirty, psf, form)
    start(fn, q, dirty, None)
    same_run(run(fn, q, form, PATCHES[0], 0.0, CYCLES), want)      # (its graph newly captured)
    for patch in PATCHES[1:]:
        assert len(fn.run_cycles(patch, 0.0, CYCLES)) == CYCLES
        assert fn.last_launches() is None                           # (not the multi-component form)
    # the first size again, from the same dirty image: its entry has been evicted, or was never stored
    start(fn, q, dirty, None)
    same_run(run(fn, q, form, PATCHES[0], 0.0, CYCLES), want)
