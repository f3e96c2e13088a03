#!/usr/bin/env python
"""Cost of a CLEAN mask: minor cycles per second of the two-launch and one-launch forms of the
device-resident loop on bench.py's CLEAN image (4096^2, 200 sources (x) PSF + noise, 111 x 133 patch,
1000 cycles), without a mask and with a random mask that allows half the pixels.

A masked cycle reads one byte per pixel of the lattice blocks on top of the 12 bytes per pixel the
cycle moves (dirty read and written, PSF read), and the loop is bound by the latency of its chain of
launches, not by those bytes: the expectation is a ratio close to 1.

    python tools/exp_clean_mask.py [--pixels 4096] [--cycles 1000] [--rounds 5]

Prints one JSON line: medians over the rounds (the variants alternate within a round).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--pixels', type=int, default=4096)
    p.add_argument('--cycles', type=int, default=1000)
    p.add_argument('--rounds', type=int, default=5)
    p.add_argument('--density', type=float, default=0.5)
    args = p.parse_args()
    from katsdpimager_amd import accel, clean, parameters
    ctx = accel.create_some_context()
    q = ctx.create_command_queue()
    G, P = args.pixels, 1
    rs = np.random.RandomState(4)          # bench.py's CLEAN image
    g1 = np.exp(-0.5 * ((np.arange(G) - G // 2) / 6.0) ** 2).astype(np.float32)
    psf = np.outer(g1, g1)[None].repeat(P, axis=0).astype(np.float32)
    psf += (0.002 * rs.standard_normal(psf.shape)).astype(np.float32)
    psf[:, G // 2, G // 2] = 1.0
    sky = (0.01 * rs.standard_normal((P, G, G))).astype(np.float32)
    for _ in range(200):
        y, x = rs.randint(100, G - 100, 2)
        amp = rs.uniform(0.5, 2.0)
        sky[:, y - 30:y + 31, x - 30:x + 31] += amp * psf[:, G // 2 - 30:G // 2 + 31,
                                                          G // 2 - 30:G // 2 + 31]
    mask = accel.DeviceArray(ctx, (G, G), np.uint8, queue=q)
    mask.set(q, (np.random.RandomState(5).uniform(size=(G, G)) < args.density).astype(np.uint8))
    fixed = parameters.FixedImageParameters(list(range(P)), np.float32)
    ip = parameters.ImageParameters(fixed, 1.0, None, 0.2, None, pixel_size=1e-5, pixels=G)
    cp = parameters.CleanParameters(args.cycles, 0.1, 0.85, 5.0, 0, 0.01, 0.5, 0.02)
    patch = (P, 111, 133)
    ops = {}
    for form in ('two_launch', 'one_launch'):
        op = clean.CleanTemplate(ctx, cp, np.float32, P, {'form': form}).instantiate(q, ip)
        op.ensure_all_bound()
        op.buffer('psf').set(q, psf)
        ops[form] = op

    def rate(form, masked):
        op = ops[form]
        op.buffer('dirty').set(q, sky)
        op.buffer('model').zero(q)
        op.bind(mask=mask if masked else None)
        op.reset()
        q.finish()
        t0 = time.perf_counter()
        op.run_cycles(patch, 0.0, args.cycles, collect=False)
        done = len(op._collect_cycle_arrays()[0])
        q.finish()
        assert done == args.cycles, done
        return done / (time.perf_counter() - t0)

    variants = [(form, masked) for form in ops for masked in (False, True)]
    for v in variants:          # graph capture and instantiation
        rate(*v)
    samples = {v: [] for v in variants}
    for _ in range(args.rounds):
        for v in variants:
            samples[v].append(rate(*v))
    out = dict(pixels=G, patch=list(patch), cycles=args.cycles, rounds=args.rounds, density=args.density)
    for form in ops:
        plain, masked = (float(np.median(samples[(form, m)])) for m in (False, True))
        out[form] = dict(unmasked_cycles_per_s=round(plain, 1), masked_cycles_per_s=round(masked, 1),
                         masked_over_unmasked=round(masked / plain, 4),
                         unmasked_spread=[round(min(samples[(form, False)]), 1), round(max(samples[(form, False)]), 1)],
                         masked_spread=[round(min(samples[(form, True)]), 1), round(max(samples[(form, True)]), 1)])
    print(json.dumps(out))


if __name__ == '__main__':
    main()
