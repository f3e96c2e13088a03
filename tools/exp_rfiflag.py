#!/usr/bin/env python3
"""Rate of the RFI flagger (rfiflag.RFIFlag, csrc/rfiflag.hip) on one MI355X, against a
device-to-device copy of the block's 12 bytes per sample (visibility and weight) in the same run.

    python tools/exp_rfiflag.py [--channels 64] [--rows 2097152] [--pols 1] [--line 0] [--run 125]
                                [--time-bin 64] [--max-window 16] [--rho 1.5] [--directions both]

Gaussian noise under weights U(0.5, 2) with a spike in one sample of a thousand.  One untimed call
through the operator (it makes and uploads the group tables and grows the workspace), then 9 timed
calls of kimg_rfi_flag on those tables, device events around each, the weights put back before each
(untimed: the operator zeroes what it flags, and a second call on its own output would have less to
do), and the median.  Prints one JSON line.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_ms(torch, stream, fn, before=None, repeats=9):
    if before:
        before()
    fn()                                    # untimed
    stream.synchronize()
    times = []
    for _ in range(repeats):
        if before:
            before()
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
    ap.add_argument('--line', type=int, default=0, help='protected channels, in the middle of the band')
    ap.add_argument('--run', type=int, default=125, help='rows per baseline')
    ap.add_argument('--time-bin', type=int, default=64)
    ap.add_argument('--max-window', type=int, default=16)
    ap.add_argument('--rho', type=float, default=1.5)
    ap.add_argument('--directions', default='both')
    args = ap.parse_args(argv)
    import torch
    from katsdpimager_amd import accel, rfiflag
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
        vis_t *= torch.where(torch.rand((C, N, P), generator=gen, device=ctx.device) < 1e-3, 20.0, 1.0)
        weights_0 = torch.rand((C, N, P), generator=gen, device=ctx.device) * 1.5 + 0.5
        weights_t = weights_0.clone()
        source = torch.empty(12 * C * N * P, dtype=torch.uint8, device=ctx.device).zero_()
        target = torch.empty_like(source)
    vis = accel.DeviceArray(ctx, (C, N, P), np.complex64, tensor=vis_t, queue=queue)
    weights = accel.DeviceArray(ctx, (C, N, P), np.float32, tensor=weights_t, queue=queue)
    baselines = (np.arange(N) // args.run).astype(np.int32)
    queue.finish()

    def copy():
        with torch.cuda.stream(stream):
            target.copy_(source)

    def restore():
        with torch.cuda.stream(stream):
            weights_t.copy_(weights_0)
    params = rfiflag.RFIFlagParameters(args.time_bin, max_window=args.max_window, rho=args.rho,
                                       directions=args.directions, line_ranges=ranges)
    op = rfiflag.RFIFlagTemplate(ctx, params).instantiate(queue, C)
    op(vis, weights, baselines)
    kept, flagged, skipped = op.counts()
    G = op.level.shape[0]
    mask = op._mask.ctypes.data_as(ctypes.c_void_p)
    factors = op._factors.ctypes.data_as(ctypes.c_void_p)

    def call():
        check(lib().kimg_rfi_flag(
            vis.ptr, N * P, weights.ptr, N * P, C, N, P, mask, op._tables.ptr, G,
            op._tables.ptr + 4 * (G + 1), params.time_bin, factors, params.max_window,
            rfiflag.DIRECTIONS[params.directions], params.level_iterations, params.level_clip,
            params.extend_freq or 0.0, params.extend_time or 0.0, int(params.extend_pols),
            op.flags.ptr, op.level.ptr, op._workspace.ptr, op._workspace.shape[0], op._counts.ptr,
            queue.handle), 'kimg_rfi_flag')
    copy_ms, _ = median_ms(torch, stream, copy)
    ms, all_ms = median_ms(torch, stream, call, before=restore)
    samples = C * N * P
    print(json.dumps(dict(
        channels=C, rows=N, pols=P, protected=args.line, time_bin=params.time_bin, groups=G,
        max_window=params.max_window, rho=params.rho, directions=params.directions,
        kept_first_call=kept, flagged_first_call=flagged, skipped_first_call=skipped,
        flagged_fraction=round(flagged / max(kept + flagged, 1), 5),
        ms=round(ms, 4), all_ms=[round(t, 4) for t in all_ms],
        gsamples_per_s=round(samples / (ms * 1e-3) / 1e9, 3),
        copy_bytes=12 * samples, copy_ms=round(copy_ms, 4),
        copy_tb_per_s=round(2 * 12 * samples / (copy_ms * 1e-3) / 1e12, 3),
        copy_time_over_time=round(copy_ms / ms, 4))))


if __name__ == '__main__':
    main()
