#!/usr/bin/env python3
"""Cost of the uv taper in the density pass (kimg_density_weights_taper against
kimg_density_weights, csrc/weight.hip) on one MI355X: the same grid, the same session, the two
calls one after the other, for DESIGN 5.16.

    python tools/exp_uv_taper.py [--size 4096] [--pols 1,4]

Best of 5 after one untimed run, device events around the call.  Both calls work in place, so every
timed run starts from a fresh device-to-device copy of the weights (outside the events).  Prints one
JSON line per polarization count: the two times, their ratio, and the pass's traffic (4 bytes read
and 4 written per cell and polarization) over each time.  ``parts_ms`` times the tapered call with
parts of the taper switched off (identity: exp(0) and the square root only; gaussian: no cuts, no
ramps; range: cuts and ramps without a Gaussian), which shows where its time goes.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def best_ms(torch, stream, prepare, fn, repeats=5):
    times = []
    for i in range(repeats + 1):
        prepare()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(stream)
        fn()
        stop.record(stream)
        stop.synchronize()
        if i:                                   # (the first run is not timed)
            times.append(start.elapsed_time(stop))
    return min(times), times


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--pols', default='1,4')
    args = ap.parse_args(argv)
    import torch
    from katsdpimager_amd import _lib, accel, weight
    lib = _lib.lib()
    G = args.size
    ctx = accel.create_some_context()
    queue = ctx.create_command_queue()
    stream = queue.stream
    image_size = 0.08
    # a 30-arcsecond beam at 30 degrees, both cuts and both ramps: every branch of the taper is live
    params = weight.UVTaperParameters.from_arcsec((30.0, 20.0), 30.0, min_uv=200.0, max_uv=20000.0,
                                                  inner_tukey=300.0, outer_tukey=4000.0)
    taper = _lib.UVTaper(*params.coefficients())
    parts = dict(identity=weight.UVTaperParameters(),
                 gaussian=weight.UVTaperParameters(params.gaussian),
                 range=weight.UVTaperParameters(None, params.min_uv, params.max_uv, params.inner_tukey,
                                                params.outer_tukey))
    step = 1.0 / image_size
    for P in (int(p) for p in args.pols.split(',')):
        with torch.cuda.stream(stream):
            gen = torch.Generator(device=ctx.device).manual_seed(1)
            source = torch.rand((P, G, G), generator=gen, device=ctx.device) * 3.0 + 1.0
            source[torch.rand((P, G, G), generator=gen, device=ctx.device) < 1.0 / 3.0] = 0.0
            work = torch.empty_like(source)
            sums = torch.zeros(3, dtype=torch.float64, device=ctx.device)

        def prepare():
            with torch.cuda.stream(stream):
                work.copy_(source)

        def plain():
            _lib.check(lib.kimg_density_weights(sums.data_ptr(), work.data_ptr(), G, G * G, G, G, P,
                                                1.0, 0.0, queue.handle), 'kimg_density_weights')

        def tapered(taper=taper):
            _lib.check(lib.kimg_density_weights_taper(
                sums.data_ptr(), work.data_ptr(), G, G * G, G, G, P, 1.0, 0.0, None, 0.0, step, step,
                ctypes.byref(taper), queue.handle), 'kimg_density_weights_taper')

        plain_ms, plain_all = best_ms(torch, stream, prepare, plain)
        taper_ms, taper_all = best_ms(torch, stream, prepare, tapered)
        parts_ms = {}
        for name, part in parts.items():
            struct = _lib.UVTaper(*part.coefficients())
            parts_ms[name] = round(best_ms(torch, stream, prepare, lambda: tapered(struct))[0], 4)
        traffic = 8.0 * P * G * G
        print(json.dumps(dict(
            size=G, pols=P, plain_ms=round(plain_ms, 4), taper_ms=round(taper_ms, 4),
            ratio=round(taper_ms / plain_ms, 3), parts_ms=parts_ms,
            plain_all_ms=[round(t, 4) for t in plain_all], taper_all_ms=[round(t, 4) for t in taper_all],
            plain_tb_per_s=round(traffic / (plain_ms * 1e-3) / 1e12, 3),
            taper_tb_per_s=round(traffic / (taper_ms * 1e-3) / 1e12, 3),
            cells_with_taper_above_0=int(np.count_nonzero(weight.uv_taper_host((G, G), image_size, params))))))


if __name__ == '__main__':
    main()
