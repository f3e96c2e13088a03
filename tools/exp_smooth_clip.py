#!/usr/bin/env python3
"""Time of the detection mask's kernels (csrc/cube_detect.hip) and of the whole smooth-and-clip finder
(detect.SmoothClip) on one MI355X, each kernel against a device-to-device copy of the bytes its model
moves, in the same process.

    python tools/exp_smooth_clip.py [--channels 64] [--pixels 4096] [--skip-finder]
    python tools/exp_smooth_clip.py --resources

Unit Gaussian noise, one polarization, a mask with 1 % of its bytes set.  Per case one untimed call,
then 9 timed calls on the same buffers, device events around each: the median and the range.  The
model of the bytes a voxel costs: boxcar 8 (+1 with a mask), reblank 4, threshold 4 (+ the mask bytes it
sets), prune 1 to 2, apply 8 + 1; ``over_copy`` is the kernel's time over that of a device-to-device
copy of as many bytes (half read, half written), measured in this run on the cube itself and scaled.
Then ``kimg_cube_smooth`` at the radii of FWHM 3 and 6 and ``kimg_cube_stats`` on their own, and the
whole finder at (0, 3, 6) x (1, 3, 7) (median of 3) with the sum of its parts next to it.  Prints one
JSON line per case.

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
                                               os.path.join(build.CSRC, 'cube_detect.hip'),
                                               '-o', os.path.join(tmp, 'cube_detect.o')]
        text = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    for block in text.split('Function Name: ')[1:]:
        name = subprocess.run(['c++filt', block.split()[0]], capture_output=True, text=True).stdout.strip()

        def number(key):
            return int(re.search(re.escape(key) + r': (\d+)', block).group(1))
        print(json.dumps(dict(
            kernel=re.sub(r'\(anonymous namespace\)::', '', name).split('(')[0],
            vgprs=number('VGPRs'), sgprs=number('SGPRs'), lds_bytes=number('LDS Size [bytes/block]'),
            waves_per_simd=number('Occupancy [waves/SIMD]'), scratch_bytes=number('ScratchSize [bytes/lane]'))))


def measure(torch, ctx, queue, C, G, finder):
    from katsdpimager_amd import accel, cube_stats, detect
    from katsdpimager_amd._lib import lib, check
    stream = queue.stream
    M = G * G
    voxels = C * M
    with torch.cuda.stream(stream):
        gen = torch.Generator(device=ctx.device).manual_seed(1)
        data = torch.randn((C, 1, G, G), generator=gen, device=ctx.device)
        out = torch.empty_like(data)
        bits = (torch.rand((C, 1, G, G), generator=gen, device=ctx.device) < 0.01).to(torch.uint8)
        scratch_mask = torch.empty_like(bits)
    array = accel.DeviceArray(ctx, (C, 1, G, G), np.float32, tensor=data, queue=queue)
    ones = np.ones(C, np.uint8)
    filled = ones.ctypes.data_as(ctypes.c_void_p)
    handle = queue.handle
    sigma = accel.DeviceArray(ctx, (C,), np.float32, queue=queue)
    sigma.set(queue, np.ones(C, np.float32))
    queue.finish()
    base = dict(channels=C, pixels=G, voxels=voxels)

    def copy():
        with torch.cuda.stream(stream):
            out.copy_(data)
    copy_ms, copy_range = timed(torch, stream, copy)
    per_byte = copy_ms / (8.0 * voxels)         # ms per byte moved (read or written) by the copy
    print(json.dumps(dict(base, case='device-to-device copy of the cube', ms=round(copy_ms, 3),
                          range_ms=copy_range, tb_per_s=round(8 * voxels / (copy_ms * 1e-3) / 1e12, 3))),
          flush=True)

    def report(case, fn, bytes_per_voxel, repeats=9, **more):
        ms, ms_range = timed(torch, stream, fn, repeats)
        print(json.dumps(dict(base, case=case, ms=round(ms, 3), range_ms=ms_range,
                              model_bytes_per_voxel=bytes_per_voxel,
                              model_tb_per_s=round(bytes_per_voxel * voxels / (ms * 1e-3) / 1e12, 3),
                              over_copy=round(ms / (per_byte * bytes_per_voxel * voxels), 2), **more)),
              flush=True)
        return ms

    for width in (1, 3, 7, 15, 31):
        for with_mask in (False, True):
            def boxcar():
                check(lib().kimg_cube_boxcar(data.data_ptr(), M, bits.data_ptr() if with_mask else None, M,
                                             out.data_ptr(), M, C, M, filled, width, 0, handle), 'boxcar')
            report('boxcar width {}{}'.format(width, ' with a mask' if with_mask else ''), boxcar,
                   9 if with_mask else 8)

    def reblank():
        check(lib().kimg_cube_reblank(out.data_ptr(), M, data.data_ptr(), M, C, M, filled, handle), 'reblank')
    report('reblank', reblank, 4)

    for threshold, what in ((5.0, 'nothing detected'), (2.0, '2.3 % detected')):
        def clip():
            check(lib().kimg_cube_threshold(data.data_ptr(), M, scratch_mask.data_ptr(), M, C, 1, G, G,
                                            filled, sigma.ptr, 1, threshold, 0, handle), 'threshold')
        report('threshold at {} sigma ({})'.format(threshold, what), clip, 4)

    for min_channels in (1, 2):
        def prune():
            with torch.cuda.stream(stream):
                scratch_mask.copy_(bits)
            check(lib().kimg_cube_mask_prune(scratch_mask.data_ptr(), M, C, M, min_channels, handle), 'prune')

        def refill():
            with torch.cuda.stream(stream):
                scratch_mask.copy_(bits)
        refill_ms, _ = timed(torch, stream, refill)
        ms, ms_range = timed(torch, stream, prune)
        print(json.dumps(dict(base, case='prune min_channels {} (less the mask copy before it)'.format(min_channels),
                              ms=round(ms - refill_ms, 3), range_ms=ms_range, model_bytes_per_voxel=1,
                              over_copy=round((ms - refill_ms) / (per_byte * voxels), 2))), flush=True)

    def apply():
        check(lib().kimg_cube_mask_apply(data.data_ptr(), M, bits.data_ptr(), M, out.data_ptr(), M, C, M,
                                         filled, 0, handle), 'apply')
    report('apply', apply, 9)

    parts = {}
    for fwhm in (3, 6):
        radius, taps = detect.gaussian_taps(fwhm)
        table = accel.DeviceArray(ctx, (C, taps.size), np.float32, queue=queue)
        table.set(queue, np.tile(taps, (C, 1)))
        radii = np.full(C, radius, np.int32)

        def smooth():
            check(lib().kimg_cube_smooth(data.data_ptr(), M, out.data_ptr(), M, C, 1, G, G, filled,
                                         radii.ctypes.data_as(ctypes.c_void_p), table.ptr, taps.size,
                                         handle), 'smooth')
        parts[fwhm] = report('kimg_cube_smooth radius {}'.format(radius), smooth, 8, repeats=3)
    words = lib().kimg_cube_stats_scratch_bytes(C, 1) // 4
    scratch = accel.DeviceArray(ctx, (words,), np.uint32, queue=queue)
    stats = accel.DeviceArray(ctx, (5, C), np.uint32, queue=queue)

    def measure_noise():
        check(lib().kimg_cube_stats(data.data_ptr(), M, C, 1, G, G, filled, 0, C, 1,
                                    cube_stats.ESTIMATORS['median_abs'], 0, None, scratch.ptr, stats.ptr,
                                    stats.ptr + 4 * C, stats.ptr + 8 * C, stats.ptr + 12 * C,
                                    stats.ptr + 16 * C, handle), 'stats')
    parts['stats'] = report('kimg_cube_stats median_abs', measure_noise, 16, repeats=3)

    if finder:
        params = detect.SmoothClipParameters()
        op = detect.SmoothClipTemplate(ctx, params).instantiate(queue, (C, 1, G, G))
        ms, ms_range = timed(torch, stream, lambda: op(array, filled=ones), repeats=3)
        print(json.dumps(dict(base, case='the finder, (0, 3, 6) x (1, 3, 7), threshold 5', ms=round(ms, 3),
                              range_ms=ms_range, smooth_ms=round(3 * (parts[3] + parts[6]), 3),
                              stats_ms=round(9 * parts['stats'], 3))), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--channels', type=int, default=64)
    ap.add_argument('--pixels', type=int, default=4096)
    ap.add_argument('--skip-finder', action='store_true')
    ap.add_argument('--resources', action='store_true')
    args = ap.parse_args(argv)
    if args.resources:
        return resources()
    import torch
    from katsdpimager_amd import accel
    ctx = accel.create_some_context()
    queue = ctx.create_command_queue()
    measure(torch, ctx, queue, args.channels, args.pixels, not args.skip_finder)


if __name__ == '__main__':
    main()
