#!/usr/bin/env python3
"""Cost of the primary-beam correction on one MI355X, three routes to the same images, for
DESIGN 5.18:

  fused    kimg_primary_beam with the images: sample and correct in one pass
  split    kimg_primary_beam sample-only, then kimg_apply_primary_beam on model and on dirty
  host     what there was before: the beam sampled with numpy on the host (sample_host), uploaded
           (64 MiB at 4096^2), then the two applies

    python tools/exp_primary_beam.py [--size 4096] [--pols 1,4] [--rounds 7] [--host-rounds 2]

The device routes are timed with device events around the calls, interleaved round by round in one
process (after one untimed round); every timed call starts from fresh copies of the images, made
outside the events.  A device-to-device copy of one polarization's two images (8 bytes read and
8 written per pixel) on the same stream is the yardstick for what the memory system gives to a plain
stream.  The host route is timed with the host clock around work that ends in a synchronise.
Prints one JSON line per polarization count: best and median times, the traffic model (4 + 16 P
bytes per pixel fused, 4 + 2 (8 P + 4) split) over the best times, and the ratios.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--pols', default='1,4')
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--host-rounds', type=int, default=2)
    ap.add_argument('--samples', type=int, default=513)
    args = ap.parse_args(argv)
    import torch
    from katsdpimager_amd import _lib, accel, primary_beam
    lib = _lib.lib()
    G = args.size
    ctx = accel.create_some_context()
    queue = ctx.create_command_queue()
    stream = queue.stream
    pixel = 1.0e-5
    lm_scale, lm_bias = pixel, -0.5 * G * pixel
    # a beam whose table ends inside the image's corners and whose cutoff radius lies inside the
    # image: kept, blanked and NaN pixels are all there
    reach = 0.6 * G * pixel
    step = reach / (args.samples - 1)
    model = primary_beam.RadialBeam.cosine_taper(0.5 * reach, 1.0e9, [1.0e9], step, reach)
    row = model.row(1.0e9)[:args.samples]
    threshold = 0.1
    inv_step = float(primary_beam.inv_step32(step))
    d_row = accel.DeviceArray(ctx, row.shape, np.float32)
    d_row.set(queue, row)
    for P in (int(p) for p in args.pols.split(',')):
        with torch.cuda.stream(stream):
            gen = torch.Generator(device=ctx.device).manual_seed(1)
            source = torch.randn((2, P, G, G), generator=gen, device=ctx.device)
            work = torch.empty_like(source)
            beam = torch.empty((G, G), dtype=torch.float32, device=ctx.device)
            copy_to = torch.empty((2, 1, G, G), dtype=torch.float32, device=ctx.device)
        model_ptr, dirty_ptr = work[0].data_ptr(), work[1].data_ptr()

        def prepare():
            with torch.cuda.stream(stream):
                work.copy_(source)

        def fused():
            _lib.check(lib.kimg_primary_beam(beam.data_ptr(), G, model_ptr, dirty_ptr, G, G * G, G, G, P,
                                             d_row.ptr, len(row), inv_step, lm_scale, lm_bias, threshold,
                                             queue.handle), 'kimg_primary_beam')

        def sample():
            _lib.check(lib.kimg_primary_beam(beam.data_ptr(), G, None, None, 0, 0, G, G, P,
                                             d_row.ptr, len(row), inv_step, lm_scale, lm_bias, threshold,
                                             queue.handle), 'kimg_primary_beam')

        def applies():
            for ptr, replacement in ((model_ptr, 0.0), (dirty_ptr, float('nan'))):
                _lib.check(lib.kimg_apply_primary_beam(ptr, G, G * G, beam.data_ptr(), G, G, G, P,
                                                       threshold, replacement, queue.handle),
                           'kimg_apply_primary_beam')

        def split():
            sample()
            applies()

        def copy():
            with torch.cuda.stream(stream):
                copy_to.copy_(source[:, :1])

        routes = dict(fused=fused, split=split, sample=sample, applies=applies, copy=copy)
        times = {name: [] for name in routes}
        for i in range(args.rounds + 1):
            for name, fn in routes.items():
                prepare()
                if name == 'applies':
                    sample()            # (the applies alone read a real beam)
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record(stream)
                fn()
                stop.record(stream)
                stop.synchronize()
                if i:                   # (the first round is not timed)
                    times[name].append(start.elapsed_time(stop))
        # the results of the two device routes agree wherever the beam is not NaN
        # (on the queue's stream, like the calls themselves)
        prepare()
        fused()
        with torch.cuda.stream(stream):
            one = work.clone()
        prepare()
        split()
        with torch.cuda.stream(stream):
            finite = ~torch.isnan(beam)
            same = bool(torch.equal(torch.nan_to_num(one[:, :, finite]),
                                    torch.nan_to_num(work[:, :, finite])))
            kept = float((beam >= threshold).float().mean())
            blank = float(torch.isnan(beam).float().mean())

        host_times = []
        for i in range(args.host_rounds):
            prepare()
            queue.finish()
            t0 = time.perf_counter()
            host_beam = primary_beam.sample_host(row, step, G, G, lm_scale, lm_bias)
            t1 = time.perf_counter()
            with torch.cuda.stream(stream):
                beam.copy_(torch.from_numpy(host_beam))
            applies()
            queue.finish()
            t2 = time.perf_counter()
            host_times.append(((t2 - t0) * 1e3, (t1 - t0) * 1e3))
        pixels = float(G) * G
        best = {name: min(t) for name, t in times.items()}
        fused_bytes, split_bytes = (4 + 16 * P) * pixels, (4 + 2 * (8 * P + 4)) * pixels
        out = dict(
            size=G, pols=P, samples=len(row), rounds=args.rounds,
            best_ms={k: round(v, 4) for k, v in best.items()},
            median_ms={k: round(statistics.median(t), 4) for k, t in times.items()},
            fused_bytes_per_pixel=4 + 16 * P, split_bytes_per_pixel=4 + 2 * (8 * P + 4),
            fused_tb_per_s=round(fused_bytes / (best['fused'] * 1e-3) / 1e12, 3),
            split_tb_per_s=round(split_bytes / (best['split'] * 1e-3) / 1e12, 3),
            copy_tb_per_s=round(16 * pixels / (best['copy'] * 1e-3) / 1e12, 3),
            split_over_fused=round(best['split'] / best['fused'], 3),
            results_equal_where_beam_finite=same,
            kept_fraction=round(kept, 4), nan_fraction=round(blank, 4))
        if host_times:
            total, sampling = min(host_times)
            out.update(host_ms=round(total, 2), host_sampling_ms=round(sampling, 2),
                       host_over_fused=round(total / best['fused'], 1))
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
