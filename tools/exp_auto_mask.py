#!/usr/bin/env python
"""Cost of the auto-mask kernels (csrc/mask.hip) on bench.py's CLEAN image (4096^2, 200 sources (x)
PSF + noise), with 1 and 4 polarizations:

* kimg_mask_threshold at 5 sigma (|I| for one polarization, the sum of squares for four), with the
  bytes it has to move -- 4 bytes per pixel and polarization read, 1 byte per pixel written -- over
  its time;
* kimg_mask_dilate at radius 0, 3, 16 and 64 on sparse seeds (that 5 sigma mask) and on dense seeds
  (a random half of the pixels), with the pixel count;
* the auto-mask step of a major cycle (threshold + dilation by 3 on the sparse seeds, as
  Imaging.auto_mask enqueues them) next to the noise estimate it follows, both as host time from
  the call to the end of the device's work;
* the overhead per major cycle in the driver: frontend.process_channel on a synthetic channel
  (examples/image_channel.py's: three point sources, `--driver-pixels`, `--driver-vis`, two major
  cycles) with auto_mask=AutoMaskParameters(5, 3) (run A) against the same call with
  clean_mask = A's mask and no auto mask (run B), (A - B) / major cycles.

Kernel times are device events around `--launches` back-to-back launches; every figure is the median
of `--rounds` rounds after a warm-up round, the variants alternating within a round.

    python tools/exp_auto_mask.py [--pixels 4096] [--rounds 5] [--launches 20] [--output FILE]

Prints one JSON line (and writes it to FILE).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

RADII = (0, 3, 16, 64)


def clean_image(G, P):
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
    return sky


def driver_overhead(ctx, args):
    """Median host milliseconds of run A, run B and (A - B) per major cycle."""
    import math
    import torch
    import synth
    from katsdpimager_amd import accel, frontend, imaging, mask, parameters, preprocess, weight
    queue = ctx.create_command_queue()
    G, block, major = args.driver_pixels, 1 << 20, 2
    obs = synth.make_observation(G, args.driver_vis, 32, 1, device=ctx.device)
    image_p, grid_p, array_p = synth.make_parameters(obs, 1, 28, degrid=True)
    uvw_wl = obs.uvw.to(torch.float64) / obs.wavelength
    vis = torch.zeros(obs.n_vis, dtype=torch.complex128, device=ctx.device)
    for (lp, mp), flux in (((40, -25), 1.0), ((-120, 60), 0.5), ((15, 200), 0.25)):
        l, m = lp * obs.pixel_size, mp * obs.pixel_size
        n = math.sqrt(1 - l * l - m * m)
        vis += flux / n * torch.exp(-2j * math.pi * (uvw_wl[:, 0] * l + uvw_wl[:, 1] * m + uvw_wl[:, 2] * (n - 1)))
    vis = vis.to(torch.complex64)[None, :, None].contiguous()
    weights = torch.ones((1, obs.n_vis, 1), dtype=torch.float32, device=ctx.device)
    torch.cuda.synchronize()
    collector = preprocess.VisibilityCollectorDevice(queue, [image_p], [grid_p], block)
    collector.add(accel.DeviceArray(ctx, (obs.n_vis, 3), np.float32, tensor=obs.uvw),
                  accel.DeviceArray(ctx, weights.shape, np.float32, tensor=weights),
                  accel.DeviceArray(ctx, vis.shape, np.complex64, tensor=vis),
                  None, None, np.ones((1, 1), np.complex64), None)
    collector.close()
    reader = collector.reader()
    weight_p = parameters.WeightParameters(weight.WeightType.ROBUST, 0.0)
    clean_p = parameters.CleanParameters(500, 0.1, 0.85, 5.0, 0, 0.01, 0.5, 0.02)
    template = imaging.ImagingTemplate(ctx, array_p, image_p.fixed, weight_p, grid_p.fixed, clean_p)
    imager = template.instantiate(queue, image_p, grid_p, block, 0, major)
    imager.ensure_all_bound()

    def run(**kwargs):
        queue.finish()
        t0 = time.perf_counter()
        stats = frontend.process_channel(reader, 0, imager, image_p, grid_p, clean_p,
                                         weight_p.weight_type, block, major, True, **kwargs)
        queue.finish()
        return (time.perf_counter() - t0) * 1e3, stats

    params = mask.AutoMaskParameters(5.0, 3)
    _, stats = run(auto_mask=params)
    fixed = accel.DeviceArray(ctx, (G, G), np.uint8, queue=queue)
    fixed.set(queue, stats['auto_mask'].get(queue))
    a, b = [], []
    for i in range(args.rounds + 1):
        ms_a, stats_a = run(auto_mask=params)
        ms_b, stats_b = run(clean_mask=fixed)
        if i:
            a.append(ms_a)
            b.append(ms_b)
    med_a, med_b = float(np.median(a)), float(np.median(b))
    return dict(pixels=G, vis=args.driver_vis, major=stats_a['major'], minor=[stats_a['minor'], stats_b['minor']],
                mask_pixels=stats_a['mask_pixels'], run_a_ms=round(med_a, 3), run_b_ms=round(med_b, 3),
                run_a_spread=[round(min(a), 3), round(max(a), 3)],
                run_b_spread=[round(min(b), 3), round(max(b), 3)],
                overhead_per_major_cycle_ms=round((med_a - med_b) / stats_a['major'], 4))


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--pixels', type=int, default=4096)
    p.add_argument('--rounds', type=int, default=5)
    p.add_argument('--launches', type=int, default=20)
    p.add_argument('--driver-pixels', type=int, default=4096)
    p.add_argument('--driver-vis', type=int, default=4_000_000)
    p.add_argument('--output')
    args = p.parse_args()
    import torch
    from katsdpimager_amd import accel, clean, mask
    ctx = accel.create_some_context()
    q = ctx.create_command_queue()
    G = args.pixels

    def device_ms(fn):
        """Milliseconds per call of `fn` over args.launches back-to-back calls (device events)."""
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        q.finish()
        start.record(q.stream)
        for _ in range(args.launches):
            fn()
        stop.record(q.stream)
        stop.synchronize()
        return start.elapsed_time(stop) / args.launches

    def host_ms(fn):
        q.finish()
        t0 = time.perf_counter()
        fn()
        q.finish()
        return (time.perf_counter() - t0) * 1e3

    out = dict(pixels=G, rounds=args.rounds, launches=args.launches, sigma=5.0)
    dense = accel.DeviceArray(ctx, (G, G), np.uint8, queue=q)
    dense.set(q, (np.random.RandomState(5).uniform(size=(G, G)) < 0.5).astype(np.uint8))
    for P, mode in ((1, clean.CLEAN_I), (4, clean.CLEAN_SUMSQ)):
        sky = clean_image(G, P)
        noise_op = clean.NoiseEstTemplate(ctx, np.float32, P).instantiate(q, sky.shape, 0.02)
        noise_op.ensure_all_bound()
        noise_op.buffer('dirty').set(q, sky)
        noise = noise_op()
        threshold = clean.power_to_metric(mode, noise * clean.noise_threshold_scale(mode, 5.0, P))
        thr = mask.MaskThresholdTemplate(ctx, np.float32, P, mode).instantiate(q, sky.shape, 0.02)
        thr.bind(image=noise_op.buffer('dirty'))
        thr.ensure_all_bound()
        dil = mask.MaskDilateTemplate(ctx).instantiate(q, (G, G))
        dil.bind(src=thr.buffer('mask'))
        dil.ensure_all_bound()
        thr(threshold)
        sparse = thr.buffer('mask')
        seeds = int(sparse.get(q).sum())

        def step():
            thr(threshold)
            dil(3, src=sparse)

        variants = {'threshold': (device_ms, lambda: thr(threshold)),
                    'step_host': (host_ms, step), 'noise_est_host': (host_ms, noise_op)}
        for name, src in (('sparse', sparse), ('dense', dense)):
            for radius in RADII:
                variants['dilate_%s_r%d' % (name, radius)] = (
                    device_ms, lambda src=src, radius=radius: dil(radius, src=src))
        samples = {name: [] for name in variants}
        for i in range(args.rounds + 1):
            for name, (timer, fn) in variants.items():
                ms = timer(fn)
                if i:                           # (round 0 warms every variant up)
                    samples[name].append(ms)
        res = {name: round(float(np.median(v)), 5) for name, v in samples.items()}
        res['spread'] = {name: [round(min(v), 5), round(max(v), 5)] for name, v in samples.items()}
        planes = 1 if mode == clean.CLEAN_I else P
        res['threshold_bytes'] = (4 * planes + 1) * G * G
        res['threshold_GBps'] = round(res['threshold_bytes'] / (res['threshold'] * 1e-3) / 1e9, 1)
        res.update(noise=float(noise), seed_pixels=seeds, mode=int(mode))
        dil(3, src=sparse)
        res['mask_pixels_r3'] = int(dil.buffer('count').get(q)[0])
        out['P%d' % P] = res
    for stage in ('kernels', 'driver'):
        if stage == 'driver':
            out['driver'] = driver_overhead(ctx, args)
        line = json.dumps(out)
        if args.output:                 # (the kernels' figures are kept if the driver stage fails)
            with open(args.output, 'w') as f:
                f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
