#!/usr/bin/env python3
"""Rate of the moment-map operator (cube.Moments, csrc/moments.hip) on one MI355X, against a
device-to-device copy of the cube's bytes in the same run.

    python tools/exp_moments.py [--channels 64] [--pixels 4096] [--pols 1]

Per requested set of moments -- (0,), (0, 1, 2) and all five -- without and with select_hanning: one
untimed call through the operator (it uploads the per-channel tables and allocates the maps), then 9
timed calls of kimg_moments on those buffers, device events around each, and the median.  The kernel
reads every voxel once (4 C M bytes) and writes 4 bytes per element and map; the copy reads and
writes the cube's bytes once each, timed the same way, so a reduction that ran at the copy's byte
rate would take about half the copy's time.  Prints one JSON line per case with the time, the bytes
read per second and the share of the copy's rate (bytes moved per second by the kernel over bytes
moved per second by the copy)."""
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
    ap.add_argument('--pixels', type=int, default=4096)
    ap.add_argument('--pols', type=int, default=1)
    ap.add_argument('--clip', type=float, default=3.0, help='cut in units of the noise (sigma 1)')
    args = ap.parse_args(argv)
    import torch
    from katsdpimager_amd import accel, cube
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
    x = 1000.0 - 2.5 * np.arange(C)
    filled = np.ones(C, np.uint8)
    queue.finish()

    def copy():
        with torch.cuda.stream(stream):
            target.copy_(data)
    cube_bytes = 4 * C * M
    for moments in ((0,), (0, 1, 2), (0, 1, 2, 8, 9)):
        for hanning in (False, True):
            params = cube.MomentParameters(moments, cut=args.clip, select_hanning=hanning)
            op = cube.MomentsTemplate(ctx, params).instantiate(queue, (C, P, G, G))
            out = op(array, coordinates=x, filled=filled)
            entered = int(out['count'].get(queue).sum())
            outputs = 0
            for key in out:
                outputs |= cube.MOMENT_BITS[key]
            pointers = [out[m].ptr if m in out else None for m in (0, 1, 2, 8, 9, 'count')]
            host_filled = filled.ctypes.data_as(ctypes.c_void_p)

            def call():
                check(lib().kimg_moments(
                    array.ptr, M, C, M, 0, C, op._tables.ptr, op._tables.ptr + 8 * C, host_filled, 2.5,
                    int(hanning), outputs, *pointers, queue.handle), 'kimg_moments')
            copy_ms, _ = median_ms(torch, stream, copy)
            ms, all_ms = median_ms(torch, stream, call)
            moved = cube_bytes + 4 * M * len(out)
            print(json.dumps(dict(
                channels=C, pols=P, pixels=G, moments=list(moments), select_hanning=hanning,
                samples_entered=entered, ms=round(ms, 4), all_ms=[round(t, 4) for t in all_ms],
                gvoxels_per_s=round(C * M / (ms * 1e-3) / 1e9, 2), bytes_moved=moved,
                tb_per_s=round(moved / (ms * 1e-3) / 1e12, 3),
                copy_ms=round(copy_ms, 4), copy_tb_per_s=round(2 * cube_bytes / (copy_ms * 1e-3) / 1e12, 3),
                share_of_copy_rate=round((moved / ms) / (2 * cube_bytes / copy_ms), 3))))


if __name__ == '__main__':
    main()
