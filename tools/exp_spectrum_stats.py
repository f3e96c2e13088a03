#!/usr/bin/env python3
"""Time of the spectrum statistics (spectrum_stats.SpectrumStats, csrc/spectrum_stats.hip) on one
MI355X, against a device-to-device copy of the cube and against kimg_moments for moment 0 -- the
one-read column pass -- in the same process.

    python tools/exp_spectrum_stats.py [--channels 64] [--pixels 4096] [--long-channels 512]
    python tools/exp_spectrum_stats.py --resources

Unit Gaussian noise, one polarization.  Per case -- each kernel form under each estimator, then the
resident form with the subtraction in place -- one untimed call, then 9 timed calls of
kimg_spectrum_stats on the same buffers, device events around each: the median and the range.
``reads`` is what the form reads of the cube (resident 1; streaming 9 for the median and 9 more for
sigma; the subtraction one more, and a write), ``read_tb_per_s`` that many cube sizes over the time.
One more row runs ``--long-channels`` channels on a smaller plane of equal voxel count (streaming).
Prints one JSON line per case.

``--resources`` needs no GPU: it compiles the unit with the library's flags and prints registers, LDS,
waves per SIMD and scratch of every kernel as the compiler reports them."""
import argparse
import ctypes
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(torch, stream, fn, repeats=9):
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
    return statistics.median(times), [round(min(times), 3), round(max(times), 3)]


def resources():
    from katsdpimager_amd import build
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [build.hipcc()] + build.FLAGS + ['-Rpass-analysis=kernel-resource-usage', '-c',
                                               os.path.join(build.CSRC, 'spectrum_stats.hip'),
                                               '-o', os.path.join(tmp, 'spectrum_stats.o')]
        text = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    for block in text.split('Function Name: ')[1:]:
        name = subprocess.run(['c++filt', block.split()[0]], capture_output=True, text=True).stdout.strip()

        def number(key):
            return int(re.search(re.escape(key) + r': (\d+)', block).group(1))
        print(json.dumps(dict(
            kernel=re.sub(r'\(anonymous namespace\)::', '', name).split('(')[0],
            vgprs=number('VGPRs'), sgprs=number('SGPRs'), lds_bytes=number('LDS Size [bytes/block]'),
            waves_per_simd=number('Occupancy [waves/SIMD]'), scratch_bytes=number('ScratchSize [bytes/lane]'))))


def measure(torch, ctx, queue, C, G, forms, with_subtract):
    from katsdpimager_amd import accel, spectrum_stats
    from katsdpimager_amd._lib import lib, check
    stream = queue.stream
    M = G * G
    with torch.cuda.stream(stream):
        gen = torch.Generator(device=ctx.device).manual_seed(1)
        data = torch.randn((C, 1, G, G), generator=gen, device=ctx.device)
        target = torch.empty_like(data)
    array = accel.DeviceArray(ctx, (C, 1, G, G), np.float32, tensor=data, queue=queue)
    ones = np.ones(C, np.uint8)
    table = ones.ctypes.data_as(ctypes.c_void_p)
    maps = accel.DeviceArray(ctx, (5, M), np.float32, queue=queue)
    tables = accel.DeviceArray(ctx, (3 * C,), np.float32, queue=queue)     # x (float64), then cut
    host = np.concatenate((np.arange(C, dtype=np.float64).view(np.float32), np.full(C, -np.inf, np.float32)))
    tables.set(queue, host)
    queue.finish()
    base = dict(channels=C, pixels=G, cube_gb=round(4 * C * M / 1e9, 3))

    def copy():
        with torch.cuda.stream(stream):
            target.copy_(data)
    copy_ms, copy_range = timed(torch, stream, copy)
    print(json.dumps(dict(base, case='device-to-device copy', ms=round(copy_ms, 3), range_ms=copy_range,
                          tb_per_s=round(8 * C * M / (copy_ms * 1e-3) / 1e12, 3))), flush=True)

    def moment0():
        check(lib().kimg_moments(array.ptr, M, C, M, 0, C, tables.ptr, tables.ptr + 8 * C, table, 1.0, 0,
                                 1, maps.ptr, None, None, None, None, None, queue.handle), 'kimg_moments')
    moment_ms, moment_range = timed(torch, stream, moment0)
    print(json.dumps(dict(base, case='kimg_moments, moment 0', ms=round(moment_ms, 3), range_ms=moment_range,
                          reads=1, read_tb_per_s=round(4 * C * M / (moment_ms * 1e-3) / 1e12, 3))), flush=True)

    step = 4 * M
    for form in forms:
        for estimator in ('median_abs', 'mad'):
            for subtract in ((False, True) if with_subtract and form == forms[0] and estimator == 'mad' else (False,)):
                def call():
                    check(lib().kimg_spectrum_stats(
                        array.ptr, M, C, M, 0, C, table, table, spectrum_stats.ESTIMATORS[estimator], 1, 31,
                        maps.ptr, maps.ptr + step, maps.ptr + 2 * step, maps.ptr + 3 * step,
                        maps.ptr + 4 * step, array.ptr if subtract else None, M,
                        spectrum_stats.FORMS[form], queue.handle), 'kimg_spectrum_stats')
                ms, ms_range = timed(torch, stream, call)
                reads = (1 if form == 'resident' else 18) + (1 if subtract else 0)
                print(json.dumps(dict(
                    base, case='{} {}{}'.format(form, estimator, ', subtract in place' if subtract else ''),
                    ms=round(ms, 3), range_ms=ms_range, reads=reads,
                    read_tb_per_s=round(reads * 4 * C * M / (ms * 1e-3) / 1e12, 3),
                    over_moment0=round(ms / moment_ms, 2))), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--channels', type=int, default=64)
    ap.add_argument('--pixels', type=int, default=4096)
    ap.add_argument('--long-channels', type=int, default=512)
    ap.add_argument('--resources', action='store_true')
    args = ap.parse_args(argv)
    if args.resources:
        return resources()
    import torch
    from katsdpimager_amd import accel, spectrum_stats
    ctx = accel.create_some_context()
    queue = ctx.create_command_queue()
    print(json.dumps(dict(resident_limit=spectrum_stats.resident_limit())), flush=True)
    forms = ('resident', 'streaming') if args.channels <= spectrum_stats.resident_limit() else ('streaming',)
    measure(torch, ctx, queue, args.channels, args.pixels, forms, True)
    if args.long_channels:
        side = int(round(args.pixels * (args.channels / args.long_channels) ** 0.5))
        measure(torch, ctx, queue, args.long_channels, side, ('streaming',), False)


if __name__ == '__main__':
    main()
