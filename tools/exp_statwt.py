#!/usr/bin/env python3
"""Rate of the statistical reweighting operator (statwt.StatWt, csrc/statwt.hip) on one MI355X,
against the traffic model of DESIGN 5.20 and a device-to-device copy of the same number of bytes in
the same run.

    python tools/exp_statwt.py [--channels 64] [--rows 2097152] [--pols 1] [--line 16] [--time-bins 1,8]

Per time_bin: one untimed call through the operator (it makes and uploads the group tables and grows
the workspace), then 9 timed calls of kimg_statwt on those tables, device events around each, and the
median.  The model bytes are 2 x 12 per fit sample (visibility and weight, read by the first two
launches) plus 8 per sample (the weight read and written by the third); the copy moves half of them
in and half out, timed the same way.  Prints one JSON line per time_bin.
"""
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
    ap.add_argument('--rows', type=int, default=2 * 1024 * 1024)
    ap.add_argument('--pols', type=int, default=1)
    ap.add_argument('--line', type=int, default=16, help='channels left out, in the middle of the band')
    ap.add_argument('--time-bins', default='1,8')
    ap.add_argument('--run', type=int, default=125, help='rows per baseline')
    args = ap.parse_args(argv)
    import torch
    from katsdpimager_amd import accel, statwt
    from katsdpimager_amd._lib import lib, check
    C, N, P = args.channels, args.rows, args.pols
    first = (C - args.line) // 2
    ranges = [(first, first + args.line)] if args.line else None
    ctx = accel.create_some_context()
    queue = ctx.create_command_queue()
    stream = queue.stream
    with torch.cuda.stream(stream):
        gen = torch.Generator(device=ctx.device).manual_seed(1)
        vis_t = torch.view_as_complex(torch.randn((C, N, P, 2), generator=gen, device=ctx.device))
        weights_t = torch.rand((C, N, P), generator=gen, device=ctx.device) * 1.5 + 0.5
    vis = accel.DeviceArray(ctx, (C, N, P), np.complex64, tensor=vis_t, queue=queue)
    weights = accel.DeviceArray(ctx, (C, N, P), np.float32, tensor=weights_t, queue=queue)
    baselines = (np.arange(N) // args.run).astype(np.int32)
    fit_channels = C - args.line
    model_bytes = (2 * 12 * fit_channels + 8 * C) * N * P
    with torch.cuda.stream(stream):
        source = torch.empty(model_bytes // 2, dtype=torch.uint8, device=ctx.device).zero_()
        target = torch.empty_like(source)
    queue.finish()

    def copy():
        with torch.cuda.stream(stream):
            target.copy_(source)
    for time_bin in (int(x) for x in args.time_bins.split(',')):
        params = statwt.StatWtParameters(time_bin, line_ranges=ranges)
        op = statwt.StatWtTemplate(ctx, params).instantiate(queue, C)
        op(vis, weights, baselines)
        kept, flagged = op.counts()
        G = op.chi2.shape[0]
        mask = op._mask.ctypes.data_as(ctypes.c_void_p)

        def call():
            check(lib().kimg_statwt(
                vis.ptr, N * P, weights.ptr, N * P, C, N, P, mask, op._tables.ptr, G,
                op._tables.ptr + 4 * (G + 1), time_bin, params.min_samples, params.chi2_range[0],
                params.chi2_range[1], op.chi2.ptr, op._workspace.ptr, op._workspace.shape[0],
                op._counts.ptr, queue.handle), 'kimg_statwt')
        copy_ms, _ = median_ms(torch, stream, copy)
        ms, all_ms = median_ms(torch, stream, call)
        copy_rate = model_bytes / (copy_ms * 1e-3)
        print(json.dumps(dict(
            channels=C, rows=N, pols=P, fit_channels=fit_channels, time_bin=time_bin, groups=G,
            kept_first_call=kept, flagged_first_call=flagged,
            ms=round(ms, 4), all_ms=[round(t, 4) for t in all_ms],
            gsamples_per_s=round(C * N * P / (ms * 1e-3) / 1e9, 3),
            model_bytes=model_bytes, model_tb_per_s=round(model_bytes / (ms * 1e-3) / 1e12, 3),
            copy_ms=round(copy_ms, 4), copy_tb_per_s=round(copy_rate / 1e12, 3),
            share_of_copy_rate=round(copy_ms / ms, 3))))


if __name__ == '__main__':
    main()
