#!/usr/bin/env python3
"""Rate of the spectral filter (spectral.SpectralFilter, csrc/spectral.hip) on one MI355X, against
its traffic model -- every input read once, every output written once, 12 (C_in + C_out) bytes per
plane element -- and a device-to-device copy that moves the same number of bytes, in the same run.

    python tools/exp_spectral.py [--channels 64] [--rows 2097152] [--pols 1] [--repeats 9]
    python tools/exp_spectral.py --resources-only        (no device needed)

Three filters: Hanning, average(4) and hanning(bin=4) -- the sliding-window, the disjoint and the
general form of the kernel.  One untimed run, then the median of --repeats timed calls, device events
around each; filter and copy alternate, so that both see the same neighbours on the machine.  Also
compiles the unit once more with the compiler's resource remarks and prints VGPRs and waves per SIMD
of every kernel.  Prints one JSON line per filter.
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def kernel_resources():
    """{kernel name: (VGPRs, waves per SIMD, scratch bytes)} of csrc/spectral.hip, from hipcc's
    -Rpass-analysis=kernel-resource-usage with the flags of the build."""
    from katsdpimager_amd import build
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [build.hipcc()] + build.FLAGS + ['-Rpass-analysis=kernel-resource-usage', '-c',
                                               os.path.join(build.CSRC, 'spectral.hip'),
                                               '-o', os.path.join(tmp, 'spectral.o')]
        text = subprocess.run(cmd, check=True, stderr=subprocess.PIPE, universal_newlines=True).stderr
    found = {}
    name = None
    for line in text.splitlines():
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            mangled = m.group(1)
            form = re.search(r'spectral_(sliding|window)_kernelI((?:L[ib]\d+E)+)E', mangled)
            name = None
            if form:
                args = re.findall(r'L[ib](\d+)E', form.group(2))
                name = 'spectral_{}_kernel<{}>'.format(form.group(1), ', '.join(args))
                found[name] = {}
            continue
        if name is None:
            continue
        for key, pattern in (('vgprs', r' VGPRs: (\d+)'), ('waves_per_simd', r'Occupancy \[waves/SIMD\]: (\d+)'),
                             ('scratch_bytes', r'ScratchSize \[bytes/lane\]: (\d+)')):
            m = re.search(pattern, line)
            if m:
                found[name][key] = int(m.group(1))
    return found


def median_ms(torch, stream, fns, repeats):
    """The median time of every function of ``fns``, called in turn ``repeats`` times after one
    untimed round."""
    for fn in fns:
        fn()
    stream.synchronize()
    times = [[] for _ in fns]
    for _ in range(repeats):
        for fn, out in zip(fns, times):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record(stream)
            fn()
            stop.record(stream)
            stop.synchronize()
            out.append(start.elapsed_time(stop))
    return [(statistics.median(t), t) for t in times]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--channels', type=int, default=64)
    ap.add_argument('--rows', type=int, default=2 * 1024 * 1024)
    ap.add_argument('--pols', type=int, default=1)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--resources-only', action='store_true')
    args = ap.parse_args(argv)
    print(json.dumps(dict(kernel_resources=kernel_resources())))
    if args.resources_only:
        return
    import torch
    from katsdpimager_amd import accel, spectral
    C, N, Q = args.channels, args.rows, args.pols
    ctx = accel.create_some_context()
    queue = ctx.create_command_queue()
    stream = queue.stream
    with torch.cuda.stream(stream):
        gen = torch.Generator(device=ctx.device).manual_seed(1)
        vis_t = torch.view_as_complex(torch.randn((C, N, Q, 2), generator=gen, device=ctx.device))
        weights_t = torch.rand((C, N, Q), generator=gen, device=ctx.device) * 1.5 + 0.5
        weights_t[torch.rand((C, N, Q), generator=gen, device=ctx.device) < 0.05] = 0.0
    vis = accel.DeviceArray(ctx, (C, N, Q), np.complex64, tensor=vis_t, queue=queue)
    weights = accel.DeviceArray(ctx, (C, N, Q), np.float32, tensor=weights_t, queue=queue)
    queue.finish()
    for label, params in (('hanning', spectral.SpectralParameters.hanning()),
                          ('average(4)', spectral.SpectralParameters.average(4)),
                          ('hanning(bin=4)', spectral.SpectralParameters.hanning(bin=4))):
        op = spectral.SpectralFilterTemplate(ctx, params).instantiate(queue, C)
        C_out = op.num_channels_out
        model_bytes = 12 * (C + C_out) * N * Q
        # a copy that reads half of the model's bytes and writes the other half
        with torch.cuda.stream(stream):
            src = torch.empty(model_bytes // 2, dtype=torch.uint8, device=ctx.device)
            src.zero_()
            dst = torch.empty_like(src)

        def copy():
            with torch.cuda.stream(stream):
                dst.copy_(src)
        (ms, all_ms), (copy_ms, all_copy_ms) = median_ms(
            torch, stream, [lambda: op(vis, weights), copy], args.repeats)
        kept, flagged = op.counts()
        print(json.dumps(dict(
            filter=label, channels_in=C, channels_out=C_out, rows=N, pols=Q,
            ms=round(ms, 4), all_ms=[round(t, 4) for t in all_ms],
            ginputs_per_s=round(C * N * Q / (ms * 1e-3) / 1e9, 2),
            model_bytes=model_bytes, model_tb_per_s=round(model_bytes / (ms * 1e-3) / 1e12, 3),
            copy_ms=round(copy_ms, 4), all_copy_ms=[round(t, 4) for t in all_copy_ms],
            copy_tb_per_s=round(model_bytes / (copy_ms * 1e-3) / 1e12, 3),
            share_of_copy_rate=round(copy_ms / ms, 3),
            kept_per_call=kept // (args.repeats + 1), flagged_per_call=flagged // (args.repeats + 1))))
        del src, dst, op


if __name__ == '__main__':
    main()
