#!/usr/bin/env python3
"""Rate of image-plane continuum subtraction (imcontsub.ImContSub, csrc/imcontsub.hip) on one MI355X,
against a device-to-device copy of the operator's own bytes in the same run.

    python tools/exp_imcontsub.py [--channels 64] [--lines 16] [--pixels 4096] [--pols 1]

Per order 0, 1 and 3, in place and out of place: one untimed call through the operator (it uploads
the per-channel tables and allocates the maps), then 9 timed calls of kimg_imcontsub on those
buffers, device events around each, and the median.  With F channels in the fit and C filled, the
kernel reads a voxel of a fit channel twice and of any other channel once and writes every voxel
once: 4 (F + 2 C) bytes per pixel, plus 12 for the three maps.  The copy moves the same 4 (F + 2 C)
bytes per pixel -- half of them read, half written -- and is timed the same way.  (In place the timed
calls subtract again from what the last one left: the same loads, sums and stores.)  Prints one JSON
line per case with the time, the bytes per second and the share of the copy's rate."""
import argparse
import ctypes
import json
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
    ap.add_argument('--lines', type=int, default=16, help='line channels, in the middle of the band')
    ap.add_argument('--pixels', type=int, default=4096)
    ap.add_argument('--pols', type=int, default=1)
    args = ap.parse_args(argv)
    import torch
    from katsdpimager_amd import accel, imcontsub
    from katsdpimager_amd._lib import lib, check
    C, P, G = args.channels, args.pols, args.pixels
    M = P * G * G
    first = (C - args.lines) // 2
    F = C - args.lines
    ctx = accel.create_some_context()
    queue = ctx.create_command_queue()
    stream = queue.stream
    per_pixel = 4 * (F + 2 * C)
    with torch.cuda.stream(stream):
        gen = torch.Generator(device=ctx.device).manual_seed(1)
        data = torch.randn((C, P, G, G), generator=gen, device=ctx.device)
        target = torch.empty_like(data)
        copy_from = torch.randn((per_pixel // 8, M), generator=gen, device=ctx.device)
        copy_to = torch.empty_like(copy_from)
    array = accel.DeviceArray(ctx, (C, P, G, G), np.float32, tensor=data, queue=queue)
    other = accel.DeviceArray(ctx, (C, P, G, G), np.float32, tensor=target, queue=queue)
    filled = np.ones(C, np.uint8)
    queue.finish()

    def copy():
        with torch.cuda.stream(stream):
            copy_to.copy_(copy_from)
    copy_bytes = 2 * copy_from.numel() * 4
    for order in (0, 1, 3):
        params = imcontsub.ImContSubParameters(order, line_ranges=[(first, first + args.lines)])
        op = imcontsub.ImContSubTemplate(ctx, params).instantiate(queue, (C, P, G, G))
        for in_place in (False, True):
            out = op(array, filled=filled, out=None if in_place else other)
            fitted = int((out['count'].get(queue) >= order + 1).sum())
            bits = sum(imcontsub.OUTPUT_BITS[key] for key in out)
            tables = params.tables(C, filled)
            host = [t.ctypes.data_as(ctypes.c_void_p) for t in tables[:3]]
            bref = [float(b) for b in tables[4]] + [0.0] * (3 - order)
            line = array if in_place else other

            def call():
                check(lib().kimg_imcontsub(
                    array.ptr, M, line.ptr, M, C, M, host[0], host[1], host[2], op._tables.ptr,
                    op._tables.ptr + 8 * C, order, *bref, 1, bits, out['continuum'].ptr, None, M,
                    out['rms'].ptr, out['count'].ptr, queue.handle), 'kimg_imcontsub')
            copy_ms, _ = median_ms(torch, stream, copy)
            ms, all_ms = median_ms(torch, stream, call)
            moved = (per_pixel + 4 * len(out)) * M
            print(json.dumps(dict(
                channels=C, fit_channels=F, pols=P, pixels=G, order=order, in_place=in_place,
                elements_fitted=fitted, ms=round(ms, 4), all_ms=[round(t, 4) for t in all_ms],
                gvoxels_per_s=round(C * M / (ms * 1e-3) / 1e9, 2), bytes_moved=moved,
                tb_per_s=round(moved / (ms * 1e-3) / 1e12, 3), copy_ms=round(copy_ms, 4),
                copy_tb_per_s=round(copy_bytes / (copy_ms * 1e-3) / 1e12, 3),
                share_of_copy_rate=round((moved / ms) / (copy_bytes / copy_ms), 3))), flush=True)


if __name__ == '__main__':
    main()
