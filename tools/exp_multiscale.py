#!/usr/bin/env python
"""Components per second of the multi-scale CLEAN operator (katsdpimager_amd/multiscale.py) next to
the Hogbom loop (clean.Clean.run_cycles) on the same image and PSF patch.

    python tools/exp_multiscale.py [--pixels 2048] [--patch 65] [--cycles 1000]

Prints one line per configuration: Hogbom, the scales [0], [0, 4, 9] and six scales up to the largest
radius the operator takes.  Each figure is the best of ``--repeats`` runs of ``--cycles`` cycles at
threshold 0, timed on the host around the call and a queue.finish(), after one untimed run (the
set-up of the scales is not in the figure; it is printed on its own).
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_field(G, seed=3):
    """Noise, twenty Gaussian blobs of FWHM 0 to 12 pixels, and a Gaussian-core PSF of centre 1."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:G, :G].astype(np.float32)
    c = G // 2
    psf = np.exp(-((yy - c) ** 2 + (xx - c) ** 2) / (2 * 2.0 ** 2)).astype(np.float32)
    psf += (0.005 * rng.standard_normal((G, G))).astype(np.float32)
    psf /= psf[c, c]
    dirty = (0.02 * rng.standard_normal((G, G))).astype(np.float32)
    for _ in range(20):
        y, x = rng.integers(G // 8, G - G // 8, 2)
        s = max(rng.uniform(0, 12), 1.0) / 2.355
        dirty += (rng.uniform(1, 10) * np.exp(-((yy - y) ** 2 + (xx - x) ** 2) / (2 * s * s))).astype(np.float32)
    return dirty[np.newaxis], psf[np.newaxis]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--pixels', type=int, default=2048)
    ap.add_argument('--patch', type=int, default=65)
    ap.add_argument('--cycles', type=int, default=1000)
    ap.add_argument('--repeats', type=int, default=3)
    args = ap.parse_args(argv)
    from katsdpimager_amd import accel, clean, multiscale, parameters
    ctx = accel.create_some_context()
    q = ctx.create_command_queue()
    G = args.pixels
    dirty, psf = make_field(G)
    patch = (1, args.patch, args.patch)
    fixed = parameters.FixedImageParameters([0], np.float32)
    ip = parameters.ImageParameters(fixed, 1.0, None, 0.2, None, pixel_size=1e-5, pixels=G)
    cp = parameters.CleanParameters(args.cycles, 0.1, 0.85, 5.0, 0, 0.01, 0.5, 0.02)
    print('image {0} x {0}, PSF patch {1} x {1}, {2} cycles per run, gain 0.1, threshold 0'.format(
        G, args.patch, args.cycles))

    def best(start, run):
        times = []
        for i in range(args.repeats + 1):
            start()
            q.finish()
            t0 = time.perf_counter()
            n = run()
            q.finish()
            times.append(time.perf_counter() - t0)
            assert n == args.cycles, n
        return args.cycles / min(times[1:])

    hog = clean.CleanTemplate(ctx, cp, np.float32, 1).instantiate(q, ip)
    hog.ensure_all_bound()
    hog.buffer('psf').set(q, psf)

    def hog_start():
        hog.buffer('dirty').set(q, dirty)
        hog.buffer('model').zero(q)
        hog.reset()
    print('Hogbom (clean.Clean.run_cycles, form auto): {:10.0f} components/s'.format(
        best(hog_start, lambda: len(hog.run_cycles(patch, 0.0, args.cycles)))))

    for scales in ([0], [0, 4, 9], [0, 4, 9, 18, 30, 50]):
        params = multiscale.MultiScaleParameters(scales)
        op = multiscale.MultiScaleCleanTemplate(ctx, cp, params, np.float32, 1).instantiate(q, ip)
        op.ensure_all_bound()
        op.buffer('psf').set(q, psf)
        setup = []

        def start():
            op.buffer('dirty').set(q, dirty)
            op.buffer('model').zero(q)
            op.reset(new_psf=not setup)
            q.finish()
            t0 = time.perf_counter()
            op.prepare(patch)
            q.finish()
            setup.append(time.perf_counter() - t0)
        rate = best(start, lambda: len(op.run_cycles(patch, 0.0, args.cycles)))
        print('multi-scale {:<24} {:10.0f} components/s   (set-up with the PSF {:.1f} ms, '
              'residuals only {:.1f} ms)'.format(str(scales) + ':', rate, setup[0] * 1e3,
                                                 min(setup[1:]) * 1e3))
        del op


if __name__ == '__main__':
    main()
