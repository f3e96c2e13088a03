#!/usr/bin/env python3
"""Rate of the phase-centre shift operator (phaseshift.PhaseShift, csrc/phaseshift.hip) on one
MI355X, against the traffic model of DESIGN 5.15 and the machine's measured HBM copy rate.

    python tools/exp_phase_shift.py [--channels 64] [--rows 2097152] [--pols 1] [--no-uvw]

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

from exp_uvcontsub import best_ms       # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--channels', type=int, default=64)
    ap.add_argument('--rows', type=int, default=2 * 1024 * 1024)
    ap.add_argument('--pols', type=int, default=1)
    ap.add_argument('--no-uvw', action='store_true', help='rotate the visibilities only')
    args = ap.parse_args(argv)
    import torch
    from katsdpimager_amd import accel, phaseshift
    C, N, Q = args.channels, args.rows, args.pols
    params = phaseshift.PhaseShiftParameters((0.93, -0.52), (0.94, -0.51))
    inv_wavelength = phaseshift.inverse_wavelengths(1.4e9 + 26123.0 * np.arange(C))
    ctx = accel.create_some_context()
    queue = ctx.create_command_queue()
    stream = queue.stream
    with torch.cuda.stream(stream):
        gen = torch.Generator(device=ctx.device).manual_seed(1)
        vis_t = torch.view_as_complex(torch.randn((C, N, Q, 2), generator=gen, device=ctx.device))
        uvw_t = (torch.rand((N, 3), generator=gen, device=ctx.device) - 0.5) * 8000.0
        scratch = torch.empty_like(vis_t)
    vis = accel.DeviceArray(ctx, (C, N, Q), np.complex64, tensor=vis_t, queue=queue)
    uvw = accel.DeviceArray(ctx, (N, 3), np.float32, tensor=uvw_t, queue=queue)
    op = phaseshift.PhaseShiftTemplate(ctx, params).instantiate(queue, inv_wavelength)
    queue.finish()

    def copy():
        with torch.cuda.stream(stream):
            scratch.copy_(vis_t)
    copy_ms, _ = best_ms(torch, stream, copy)
    copy_rate = 2 * vis_t.numel() * 8 / (copy_ms * 1e-3)
    ms, all_ms = best_ms(torch, stream, lambda: op(vis, uvw, write_uvw=not args.no_uvw))
    model_bytes = 16 * C * N * Q + (12 if args.no_uvw else 24) * N
    print(json.dumps(dict(
        channels=C, rows=N, pols=Q, write_uvw=not args.no_uvw,
        ms=round(ms, 4), all_ms=[round(t, 4) for t in all_ms],
        gsamples_per_s=round(C * N * Q / (ms * 1e-3) / 1e9, 3),
        model_bytes=model_bytes, model_tb_per_s=round(model_bytes / (ms * 1e-3) / 1e12, 3),
        copy_ms=round(copy_ms, 4), copy_tb_per_s=round(copy_rate / 1e12, 3),
        share_of_copy_rate=round(model_bytes / (ms * 1e-3) / copy_rate, 3))))


if __name__ == '__main__':
    main()
