#!/usr/bin/env python3
"""Time of source linking (csrc/cube_link.hip, link.Link) on one MI355X.

    python tools/exp_link.py [--channels 64] [--pixels 4096] [--smooth-clip] [--host-pixels 512]
    python tools/exp_link.py --kernels DIR       (the same under rocprofv3 --kernel-trace --stats)
    python tools/exp_link.py --resources

Unit Gaussian noise, one polarization.  The mask: 1 % set in compact blobs of 4 x 8 x 8 voxels plus
0.1 % isolated voxels (the default), ``detect.SmoothClip``'s own with ``--smooth-clip``, and every voxel
of the first ``--one-source-pixels`` squared pixels of every channel set (one source).  Per case one untimed call, then 9 timed ones on the same buffers, device events
around each: the median and the range, for each of the four entries and for the whole operator call
(which ends in its one read of the tables).  ``over_copy`` is an entry's time over that of a
device-to-device copy of the bytes its model moves -- link: init 1 + 4, merge 1, flatten 1, number 1,
relabel 1 a voxel = 9 (the sparse label traffic of set voxels is not in the model); measure 4 (+ 4
where a source is); filter 4; label mask 4 + 1 -- measured in this run.  The entries' kernels one by
one come from ``--kernels``, which starts this script once more under ``rocprofv3 --kernel-trace
--stats`` and prints the rows of its kernel statistics.  The host route that the operator replaces --
the mask read back, then ``link.link_host`` and scipy's ``label`` -- is timed on a ``--host-pixels``
square part of the cube (the twins need some 40 bytes a voxel) next to the read-back of the whole mask.

``--resources`` needs no GPU: registers, LDS, waves per SIMD and scratch of every kernel as the compiler
reports them."""
import argparse
import ctypes
import glob
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

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
                                               os.path.join(build.CSRC, 'cube_link.hip'),
                                               '-o', os.path.join(tmp, 'cube_link.o')]
        text = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    for block in text.split('Function Name: ')[1:]:
        name = subprocess.run(['c++filt', block.split()[0]], capture_output=True, text=True).stdout.strip()

        def number(key):
            return int(re.search(re.escape(key) + r': (\d+)', block).group(1))
        print(json.dumps(dict(
            kernel=re.sub(r'\(anonymous namespace\)::', '', name).split('(')[0],
            vgprs=number('VGPRs'), sgprs=number('SGPRs'), lds_bytes=number('LDS Size [bytes/block]'),
            waves_per_simd=number('Occupancy [waves/SIMD]'), scratch_bytes=number('ScratchSize [bytes/lane]'))))


def synthetic_mask(torch, device, C, G, gen):
    blobs = torch.rand((C // 4 + 1, G // 8 + 1, G // 8 + 1), generator=gen, device=device) < 0.01
    blobs = blobs.repeat_interleave(4, 0).repeat_interleave(8, 1).repeat_interleave(8, 2)[:C, :G, :G]
    mask = blobs.to(torch.uint8).reshape(C, 1, G, G).contiguous()
    for c in range(C):
        mask[c, 0] |= (torch.rand((G, G), generator=gen, device=device) < 0.001).to(torch.uint8)
    return mask


def measure(torch, ctx, queue, C, G, smooth_clip, host_pixels, one_pixels, repeats):
    from katsdpimager_amd import accel, detect, link
    from katsdpimager_amd._lib import lib, check
    stream = queue.stream
    M = G * G
    shape = (C, 1, G, G)
    with torch.cuda.stream(stream):
        gen = torch.Generator(device=ctx.device).manual_seed(1)
        data = torch.randn(shape, generator=gen, device=ctx.device)
        spare = torch.empty(C * M * 9, dtype=torch.uint8, device=ctx.device)
    array = accel.DeviceArray(ctx, shape, np.float32, tensor=data, queue=queue)
    ones = np.ones(C, np.uint8)
    filled = ones.ctypes.data_as(ctypes.c_void_p)
    handle = queue.handle
    base = dict(channels=C, pixels=G, voxels=C * M)

    def copy_time(bytes_per_voxel):
        half = C * M * bytes_per_voxel // 2

        def copy():
            with torch.cuda.stream(stream):
                spare[half:2 * half].copy_(spare[:half])
        return timed(torch, stream, copy, repeats)[0]

    copies = {n: copy_time(n) for n in (4, 5, 9)}
    for n, ms in copies.items():
        print(json.dumps(dict(base, case='copy', bytes_per_voxel=n, ms=round(ms, 3))), flush=True)

    masks = {}
    if smooth_clip:
        finder = detect.SmoothClipTemplate(ctx, detect.SmoothClipParameters()).instantiate(queue, shape)
        masks['smooth_clip'] = finder(array, filled=ones)
        del finder
    else:
        with torch.cuda.stream(stream):
            tensor = synthetic_mask(torch, ctx.device, C, G, gen)
        masks['blobs'] = accel.DeviceArray(ctx, shape, np.uint8, tensor=tensor, queue=queue)
    with torch.cuda.stream(stream):
        # every voxel of the first one_pixels^2 pixels of every channel: one source
        tensor = torch.zeros(shape, dtype=torch.uint8, device=ctx.device)
        tensor[:, :, :one_pixels, :one_pixels] = 1
        masks['one_source'] = accel.DeviceArray(ctx, shape, np.uint8, queue=queue, tensor=tensor)
    queue.finish()

    params = link.LinkParameters(min_voxels=2, max_sources=2 ** 21)
    op = link.LinkTemplate(ctx, params).instantiate(queue, shape)
    labels = accel.DeviceArray(ctx, shape, np.int32, queue=queue)
    out_mask = accel.DeviceArray(ctx, shape, np.uint8, queue=queue)
    counts = op._tables.ptr
    catalogue = ctypes.byref(op._catalogue)
    rows = params.max_sources

    def host_route(name):
        # the host route, on a part
        start = time.perf_counter()
        whole_mask = masks[name].get(queue)
        readback = time.perf_counter() - start
        part = np.ascontiguousarray(whole_mask[:, :, :host_pixels, :host_pixels])
        del whole_mask
        start = time.perf_counter()
        _, found = link.link_host(part, ones, params.reach_xy_sq, params.radius_z)
        twin = time.perf_counter() - start
        row = dict(base, mask=name, entry='host', readback_ms=round(1e3 * readback, 1), part_voxels=part.size,
                   part_sources=found, link_host_ms=round(1e3 * twin, 1))
        try:
            from scipy import ndimage
            structure = np.zeros((3, 3, 3, 3), bool)
            structure[:, 1] = ndimage.generate_binary_structure(2, 1)
            start = time.perf_counter()
            ndimage.label(part, structure)
            row['scipy_label_ms'] = round(1e3 * (time.perf_counter() - start), 1)
        except ImportError:
            row['scipy_label_ms'] = None
        print(json.dumps(row), flush=True)

    for name, mask in masks.items():
        set_share = float(mask.tensor.count_nonzero().item()) / (C * M)

        def run_link():
            check(lib().kimg_cube_link(mask.ptr, M, labels.ptr, M, C, 1, G, G, filled, params.reach_xy_sq,
                                       params.radius_z, op._scratch.ptr, counts, handle), 'link')

        def run_measure():
            check(lib().kimg_cube_measure(labels.ptr, M, array.ptr, M, C, 1, G, G, filled, catalogue, rows,
                                          counts, handle), 'measure')

        def run_filter():
            check(lib().kimg_cube_link_filter(labels.ptr, M, C, M, catalogue, rows, 2, 1, 1, counts, handle),
                  'filter')

        def run_label_mask():
            check(lib().kimg_cube_label_mask(labels.ptr, M, out_mask.ptr, M, C, M, 0, handle), 'label_mask')

        case = dict(base, mask=name, set_share=round(set_share, 5))
        for entry, fn, model in (('link', run_link, 9), ('measure', run_measure, 4), ('filter', run_filter, 4),
                                 ('label_mask', run_label_mask, 5)):
            ms, spread = timed(torch, stream, fn, 3 if name == 'one_source' else repeats)
            print(json.dumps(dict(case, entry=entry, ms=round(ms, 3), range=spread, model_bytes_per_voxel=model,
                                  over_copy=round(ms / copies[model], 2))), flush=True)
        linked = int(op._tables.get(queue)[:4].view(np.int32)[0])
        print(json.dumps(dict(case, sources=linked)), flush=True)
        if linked <= rows:
            def whole():
                op(mask, array, filled=ones)
            ms, spread = timed(torch, stream, whole, min(repeats, 3))
            print(json.dumps(dict(case, entry='operator', ms=round(ms, 3), range=spread)), flush=True)
        if name != 'one_source':
            host_route(name)

def kernels(directory, argv):
    """This script again, under rocprofv3's kernel trace; prints the statistics of the unit's kernels."""
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', directory, '--', sys.executable,
           os.path.abspath(__file__)] + argv + ['--repeats', '3']
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
    for path in glob.glob(os.path.join(directory, '**', '*kernel_stats.csv'), recursive=True):
        with open(path) as f:
            for k, line in enumerate(f):
                if k == 0 or 'lk_' in line:
                    print(line.rstrip())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--channels', type=int, default=64)
    ap.add_argument('--pixels', type=int, default=4096)
    ap.add_argument('--host-pixels', type=int, default=512)
    ap.add_argument('--one-source-pixels', type=int, default=1024)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--smooth-clip', action='store_true')
    ap.add_argument('--kernels', metavar='DIR')
    ap.add_argument('--resources', action='store_true')
    args = ap.parse_args()
    if args.resources:
        return resources()
    if args.kernels:
        rest = ['--channels', str(args.channels), '--pixels', str(args.pixels), '--host-pixels', '64']
        return kernels(args.kernels, rest + (['--smooth-clip'] if args.smooth_clip else []))
    import torch
    from katsdpimager_amd import accel
    ctx = accel.Context(0)
    queue = ctx.create_command_queue()
    measure(torch, ctx, queue, args.channels, args.pixels, args.smooth_clip, min(args.host_pixels, args.pixels),
            min(args.one_source_pixels, args.pixels), args.repeats)


if __name__ == '__main__':
    main()
