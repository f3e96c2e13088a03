#!/usr/bin/env python3
"""Rate of cube smoothing to a common beam (smooth.CubeSmooth, csrc/cube_smooth.hip) on one MI355X,
against a device-to-device copy of the same 8 bytes per voxel in the same run, and at R = 2 and
R = 8 against beam.ConvolveBeam plane by plane on the same cube -- the route a caller would
otherwise take.

    python tools/exp_cube_smooth.py [--channels 64] [--pixels 4096] [--pols 1]

Per case -- a uniform R of 0, 1, 2, 4, 8 and 16 (round beams of sigma 2 px taken to the beam whose
kernel has sigma just under R / 4), and the mixed radii of a 5 % band (beams of sigma 2 px that
scale with 1 / f, taken to the largest) -- one untimed call through the operator (it uploads the
taps), then 9 timed calls of kimg_cube_smooth on those buffers, device events around each, and the
median.  The kernel reads every voxel once from the cube (halos come again through the caches) and
writes it once: 8 bytes per voxel.  The copy moves the cube into the second buffer and is timed the
same way.  The FFT route copies a plane into ConvolveBeam's image, convolves it in place and copies
it into the second buffer, all planes of the cube between one pair of events.  Prints one JSON line
per case."""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_ms(torch, stream, fn, repeats=9):
    fn()                                    # untimed
    stream.synchronize()
    times = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(stream)
        fn()
        stop.record(stream)
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    return statistics.median(times), times


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--channels', type=int, default=64)
    ap.add_argument('--pixels', type=int, default=4096)
    ap.add_argument('--pols', type=int, default=1)
    ap.add_argument('--no-fft', action='store_true', help='skip the ConvolveBeam route')
    args = ap.parse_args(argv)
    import torch
    from katsdpimager_amd import accel, beam, smooth
    from katsdpimager_amd._lib import lib, check
    C, P, G = args.channels, args.pols, args.pixels
    M = P * G * G
    ctx = accel.create_some_context()
    queue = ctx.create_command_queue()
    stream = queue.stream
    with torch.cuda.stream(stream):
        gen = torch.Generator(device=ctx.device).manual_seed(1)
        data = torch.randn((C, P, G, G), generator=gen, device=ctx.device)
        target = torch.empty_like(data)
    array = accel.DeviceArray(ctx, (C, P, G, G), np.float32, tensor=data, queue=queue)
    other = accel.DeviceArray(ctx, (C, P, G, G), np.float32, tensor=target, queue=queue)
    filled = np.ones(C, np.uint8)
    queue.finish()
    moved = 8 * C * M

    def copy():
        with torch.cuda.stream(stream):
            target.copy_(data)
    cases = []
    for R in (0, 1, 2, 4, 8, 16):
        sigma = 0.999 * R / 4.0
        to = beam.Beam(1.0, math.sqrt(4.0 + sigma ** 2), math.sqrt(4.0 + sigma ** 2), 0.0)
        cases.append(('R = {}'.format(R), [beam.Beam(1.0, 2.0, 2.0, 0.0)] * C, to, sigma))
    frequencies = 1.4e9 * (1.0 + 0.05 * np.arange(C) / max(C - 1, 1))
    cases.append(('5 % band', [beam.Beam(1.0, 2.0 * frequencies[0] / f, 2.0 * frequencies[0] / f, 0.0)
                               for f in frequencies], None, None))
    convolve = None
    for name, beams, to, sigma in cases:
        op = smooth.CubeSmoothTemplate(ctx, smooth.CommonBeamParameters(to)).instantiate(queue, (C, P, G, G))
        op(array, beams=beams, filled=filled, out=other)
        radius = op.radius

        def call():
            check(lib().kimg_cube_smooth(
                array.ptr, M, other.ptr, M, C, P, G, G, filled.ctypes.data_as(ctypes.c_void_p),
                radius.ctypes.data_as(ctypes.c_void_p), op._taps.ptr, smooth.TAPS_PITCH,
                queue.handle), 'kimg_cube_smooth')
        copy_ms, _ = median_ms(torch, stream, copy)
        ms, all_ms = median_ms(torch, stream, call)
        line = dict(
            case=name, channels=C, pols=P, pixels=G, radius_min=int(radius.min()),
            radius_max=int(radius.max()), ms=round(ms, 4), all_ms=[round(t, 4) for t in all_ms],
            gvoxels_per_s=round(C * M / (ms * 1e-3) / 1e9, 2),
            tb_per_s=round(moved / (ms * 1e-3) / 1e12, 3), copy_ms=round(copy_ms, 4),
            copy_tb_per_s=round(moved / (copy_ms * 1e-3) / 1e12, 3),
            share_of_copy_rate=round(copy_ms / ms, 3))
        if sigma is not None and name in ('R = 2', 'R = 8') and not args.no_fft:
            if convolve is None:
                convolve = beam.ConvolveBeamTemplate(ctx, (G, G), np.float32).instantiate(queue)
                convolve.ensure_all_bound()
            convolve.beam = beam.Beam(1.0, sigma, sigma, 0.0)
            image = convolve.buffer('image')

            def fft_route():
                for c in range(C):
                    for p in range(P):
                        array.copy_region(queue, image, np.s_[c, p], ())
                        convolve()
                        image.copy_region(queue, other, (), np.s_[c, p])
            fft_ms, fft_all = median_ms(torch, stream, fft_route)
            line.update(fft_route_ms=round(fft_ms, 3), fft_route_all_ms=[round(t, 3) for t in fft_all],
                        fft_route_over_direct=round(fft_ms / ms, 2))
        print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
