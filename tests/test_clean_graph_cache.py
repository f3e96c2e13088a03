"""The cache of captured minor-cycle graphs (csrc/kimg_graph_cache.h) past its capacity: 32 argument
sets.  Forty PSF patch sizes on one set of buffers are forty argument sets, and every call of 64
cycles asks for a graph (64 >= KIMG_GRAPH_CYCLES / 2), so at least eight of the calls have to evict
an entry or fall back to plain launches.  Whichever it was, a call whose entry is gone gives what
the per-call form (no graphs) gives, bit for bit.

The same walk through the multi-component form fills the other cache (clean_multi.hip), and four host
threads with an imager and a stream each fill the first one together: 48 argument sets, captured,
replayed, evicted and released concurrently.  (The cache's rules themselves -- what may be evicted,
what a failed capture leaves behind -- are tested on the host, test_graph_cache_host.py.)"""
import functools
import threading
import time

import numpy as np
import pytest

from test_clean_mask import BORDER, G, make_clean, problem, run, same_run, start

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


@gpu
def test_more_argument_sets_than_slots_multi():
    """The walk in the multi-component form, one component and one step per launch: every call needs
    64 launches or more, which go out as graphs of 16 (MULTI_GRAPH) from multi_cache -- with the
    form's own caps (8 components, repeated steps) a call of 64 cycles is over before it asks for a
    graph."""
    from test_clean_multi_gpu import _check, _clean
    psf, dirty, want = per_call()
    fn, q = _clean(G, P, MODE, BORDER, 0.1, dirty, psf, {'form': 'multi', 'components': 1, 'repeats': 1})
    _check(fn, q, fn.run_cycles(PATCHES[0], 0.0, CYCLES), want)
    assert fn.last_launches() >= CYCLES
    for patch in PATCHES[1:]:
        assert len(fn.run_cycles(patch, 0.0, CYCLES)) == CYCLES
        assert fn.last_launches() >= CYCLES                         # (the multi-component form)
    start(fn, q, dirty, None)
    _check(fn, q, fn.run_cycles(PATCHES[0], 0.0, CYCLES), want)
    assert fn.last_launches() >= CYCLES


THREADS = 4
JOIN_TIMEOUT = 60.0     # seconds for all threads together; they need about one


@gpu
def test_threads_share_the_cache():
    """Four threads, each with its own imager, buffers and stream, each walking 12 patch sizes in the
    one-launch form: 48 argument sets for 32 slots, and the library calls overlap (ctypes releases the
    GIL).  Every thread's first run, and the same run again after its walk, is the single-threaded
    per-call result bit for bit; every call in between returns its 64 cycles."""
    import torch
    from helpers import context_queue
    from katsdpimager_amd import clean, parameters
    psf, dirty, want = per_call()
    ctx, _ = context_queue()
    fixed = parameters.FixedImageParameters(list(range(P)), np.float32)
    ip = parameters.ImageParameters(fixed, 1.0, None, 0.2, None, pixel_size=1e-5, pixels=G)
    cp = parameters.CleanParameters(1000, 0.1, 0.85, 5.0, MODE, 0.01, 0.5, BORDER)
    workers = []
    for t in range(THREADS):
        q = ctx.create_command_queue()                              # a stream of its own
        fn = clean.CleanTemplate(ctx, cp, np.float32, P, {'form': 'one_launch'}).instantiate(q, ip)
        fn.ensure_all_bound()
        fn.buffer('psf').set(q, psf)
        q.finish()
        workers.append((fn, q, [PATCHES[0]] + PATCHES[1 + 9 * t:12 + 9 * t]))
    assert all(len(set(w[2])) == 12 for w in workers) and THREADS * 12 > 32
    assert len({w[1].handle for w in workers}) == THREADS
    results, errors = {}, []
    go = threading.Barrier(THREADS)

    def work(t):
        try:
            fn, q, patches = workers[t]
            with torch.cuda.device(ctx.device):
                go.wait(JOIN_TIMEOUT)
                start(fn, q, dirty, None)
                first = run(fn, q, 'one_launch', patches[0], 0.0, CYCLES)
                counts = [len(fn.run_cycles(patch, 0.0, CYCLES)) for patch in patches[1:]]
                start(fn, q, dirty, None)
                results[t] = (first, counts, run(fn, q, 'one_launch', patches[0], 0.0, CYCLES))
        except Exception as exc:        # noqa: B902
            errors.append((t, exc))

    threads = [threading.Thread(target=work, args=(t,), daemon=True) for t in range(THREADS)]
    for th in threads:
        th.start()
    deadline = time.monotonic() + JOIN_TIMEOUT
    for th in threads:
        th.join(max(0.0, deadline - time.monotonic()))
    assert not any(th.is_alive() for th in threads), 'a thread did not come back'
    assert not errors, errors
    for t in range(THREADS):
        first, counts, last = results[t]
        assert counts == [CYCLES] * 11
        same_run(first, want)
        same_run(last, want)
        assert workers[t][0].last_launches() is None                # (not the multi-component form)
