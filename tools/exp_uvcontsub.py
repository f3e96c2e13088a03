#!/usr/bin/env python3
"""Rate of the UV-plane continuum subtraction operator (continuum.UVContSub, csrc/contsub.hip) on
one MI355X, against the traffic model of DESIGN 5.14 and the machine's measured HBM copy rate.

    python tools/exp_uvcontsub.py [--channels 64] [--rows 2097152] [--pols 1] [--order 1] [--line 16]

Best of 5 after one untimed run, device events around the call.  The copy rate is a device-to-device
copy of the visibility block (bytes read + bytes written over the best of 5), measured the same way.
Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def best_ms(torch, stream, fn, repeats=5):
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
    return min(times), times


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--channels', type=int, default=64)
    ap.add_argument('--rows', type=int, default=2 * 1024 * 1024)
    ap.add_argument('--pols', type=int, default=1)
    ap.add_argument('--order', type=int, default=1)
    ap.add_argument('--line', type=int, default=16, help='channels masked out, in the middle of the band')
    args = ap.parse_args(argv)
    import torch
    from katsdpimager_amd import accel, continuum
    C, N, Q = args.channels, args.rows, args.pols
    first = (C - args.line) // 2
    params = continuum.UVContSubParameters(args.order, line_ranges=[(first, first + args.line)])
    ctx = accel.create_some_context()
    queue = ctx.create_command_queue()
    stream = queue.stream
    with torch.cuda.stream(stream):
        gen = torch.Generator(device=ctx.device).manual_seed(1)
        vis_t = torch.view_as_complex(torch.randn((C, N, Q, 2), generator=gen, device=ctx.device))
        weights_t = torch.rand((C, N, Q), generator=gen, device=ctx.device) * 1.5 + 0.5
        scratch = torch.empty_like(vis_t)
    vis = accel.DeviceArray(ctx, (C, N, Q), np.complex64, tensor=vis_t, queue=queue)
    weights = accel.DeviceArray(ctx, (C, N, Q), np.float32, tensor=weights_t, queue=queue)
    op = continuum.UVContSubTemplate(ctx, params).instantiate(queue, C)
    queue.finish()

    def copy():
        with torch.cuda.stream(stream):
            scratch.copy_(vis_t)
    copy_ms, _ = best_ms(torch, stream, copy)
    copy_rate = 2 * vis_t.numel() * 8 / (copy_ms * 1e-3)
    ms, all_ms = best_ms(torch, stream, lambda: op(vis, weights))
    fitted, flagged = op.counts()
    fit_channels = C - args.line
    model_bytes = (12 * fit_channels + 16 * C) * N * Q
    print(json.dumps(dict(
        channels=C, rows=N, pols=Q, order=args.order, fit_channels=fit_channels,
        ms=round(ms, 4), all_ms=[round(t, 4) for t in all_ms],
        gsamples_per_s=round(C * N * Q / (ms * 1e-3) / 1e9, 3),
        model_bytes=model_bytes, model_tb_per_s=round(model_bytes / (ms * 1e-3) / 1e12, 3),
        copy_ms=round(copy_ms, 4), copy_tb_per_s=round(copy_rate / 1e12, 3),
        share_of_copy_rate=round(model_bytes / (ms * 1e-3) / copy_rate, 3),
        fitted_per_call=fitted // 6, flagged=flagged)))


if __name__ == '__main__':
    main()
