#!/usr/bin/env python3
"""Time of the cube plane statistics (cube_stats.CubeStats, csrc/cube_stats.hip) on one MI355X,
against a device-to-device copy of the cube in the same run and against clean.NoiseEst's
kimg_noise_est called plane by plane on the same cube -- the only route there was.

    python tools/exp_cube_stats.py [--channels 64] [--pixels 4096] [--pols 1]
    python tools/exp_cube_stats.py --resources

Noise-like data (unit Gaussian).  Per case -- both estimators, without and with a region (a disc of
half the plane's width, as a primary beam's ``beam_valid``; a region takes the form that makes (y, x)
from the element index) -- one untimed call, then 9 timed calls of kimg_cube_stats on the same
buffers, device events around each, and the median.  'median_abs' reads the cube 4 times, 'mad' 8
times; ``reads_at_copy_rate_ms`` is what that many reads cost at the rate the copy reached (the copy
reads and writes: 8 bytes a voxel).  The plane-by-plane loop is C * P calls of kimg_noise_est (9
launches each, 4 reads of the plane) between one pair of events, without the 4-byte read-back that
clean.NoiseEst adds to each.  Prints one JSON line per case.

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


def resources():
    from katsdpimager_amd import build
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [build.hipcc()] + build.FLAGS + ['-Rpass-analysis=kernel-resource-usage', '-c',
                                               os.path.join(build.CSRC, 'cube_stats.hip'),
                                               '-o', os.path.join(tmp, 'cube_stats.o')]
        text = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    for block in text.split('Function Name: ')[1:]:
        name = subprocess.run(['c++filt', block.split()[0]], capture_output=True, text=True).stdout.strip()

        def number(key):
            return int(re.search(re.escape(key) + r': (\d+)', block).group(1))
        print(json.dumps(dict(
            kernel=re.sub(r'\(anonymous namespace\)::', '', name).split('(')[0],
            vgprs=number('VGPRs'), sgprs=number('SGPRs'), lds_bytes=number('LDS Size [bytes/block]'),
            waves_per_simd=number('Occupancy [waves/SIMD]'), scratch_bytes=number('ScratchSize [bytes/lane]'))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--channels', type=int, default=64)
    ap.add_argument('--pixels', type=int, default=4096)
    ap.add_argument('--pols', type=int, default=1)
    ap.add_argument('--resources', action='store_true')
    args = ap.parse_args(argv)
    if args.resources:
        return resources()
    import torch
    from katsdpimager_amd import accel, clean, cube_stats
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
    filled = np.ones(C, np.uint8)
    y, x = np.mgrid[:G, :G]
    disc = ((y - G // 2) ** 2 + (x - G // 2) ** 2 <= (G // 4) ** 2).astype(np.uint8)
    region = accel.DeviceArray(ctx, (G, G), np.uint8, queue=queue)
    region.set(queue, disc)
    queue.finish()

    def copy():
        with torch.cuda.stream(stream):
            target.copy_(data)
    copy_ms, _ = median_ms(torch, stream, copy)
    read_ms = copy_ms / 2                   # one read of the cube at the copy's rate

    scratch = accel.DeviceArray(ctx, (lib().kimg_noise_est_scratch_bytes() // 4,), np.uint32, queue=queue)
    single = accel.DeviceArray(ctx, (C * P,), np.float32, queue=queue)
    to_rms = float(np.float32(clean._MEDIAN_TO_RMS))

    def plane_by_plane():
        for c in range(C):
            for p in range(P):
                check(lib().kimg_noise_est(array.ptr + 4 * (c * M + p * G * G), G, G * G, G, G, 1, 0,
                                           to_rms, scratch.ptr, single.ptr + 4 * (c * P + p),
                                           queue.handle), 'kimg_noise_est')
    loop_ms, loop_all = median_ms(torch, stream, plane_by_plane)
    loop_sigma = single.get(queue)
    print(json.dumps(dict(case='kimg_noise_est plane by plane', channels=C, pols=P, pixels=G,
                          ms=round(loop_ms, 3), all_ms=[round(t, 3) for t in loop_all],
                          copy_ms=round(copy_ms, 3), reads_at_copy_rate_ms=round(4 * read_ms, 3))), flush=True)

    for estimator, reads in (('median_abs', 4), ('mad', 8)):
        for with_region in (False, True):
            params = cube_stats.CubeStatsParameters(estimator=estimator, pool_polarizations=False)
            op = cube_stats.CubeStatsTemplate(ctx, params).instantiate(queue, (C, P, G, G))
            result = op(array, filled=filled, region=region if with_region else None)
            out = op._out.ptr
            step = 4 * C * P

            def call():
                check(lib().kimg_cube_stats(
                    array.ptr, M, C, P, G, G, filled.ctypes.data_as(ctypes.c_void_p), 0, C, 0,
                    cube_stats.ESTIMATORS[estimator], 0, region.ptr if with_region else None,
                    op._scratch.ptr, out, out + step, out + 2 * step, out + 3 * step, out + 4 * step,
                    queue.handle), 'kimg_cube_stats')
            ms, all_ms = median_ms(torch, stream, call)
            line = dict(case=estimator + (' in a region' if with_region else ''), channels=C, pols=P,
                        pixels=G, ms=round(ms, 3), all_ms=[round(t, 3) for t in all_ms], reads=reads,
                        read_tb_per_s=round(reads * 4 * C * M / (ms * 1e-3) / 1e12, 3),
                        copy_ms=round(copy_ms, 3), reads_at_copy_rate_ms=round(reads * read_ms, 3),
                        loop_over_batched=round(loop_ms / ms, 2),
                        sigma_mean=float(result.sigma.mean()))
            if estimator == 'median_abs' and not with_region:
                line['same_bits_as_loop'] = bool(np.array_equal(
                    result.sigma.reshape(-1).view(np.uint32), loop_sigma.view(np.uint32)))
            print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
