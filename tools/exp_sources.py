#!/usr/bin/env python3
"""Time of the source spectra and line parameters (csrc/cube_sources.hip, sources.Sources) on one MI355X.

    python tools/exp_sources.py [--channels 64] [--pixels 4096] [--one-source-pixels 1024] [--repeats 9]
    python tools/exp_sources.py --resources

Unit Gaussian noise, one polarization.  Two inputs: ``exp_link.py``'s mask -- 1 % set in compact blobs
of 4 x 8 x 8 voxels plus 0.1 % isolated voxels, about a million sources -- linked on the device, and
``exp_link.py``'s one-source input: every voxel of the first ``--one-source-pixels`` squared pixels of
every channel set, 67 million voxels in one source, every lane of a wave on one label.  Per input one
untimed call, then ``--repeats`` timed ones on the same buffers, device events around each: the median
and the range of ``kimg_cube_source_spectra``, of
``kimg_cube_measure`` on the same labels and cube, and of ``kimg_source_lines``.  In the same run a
device-to-device copy of the 8 bytes a voxel that the spectra pass reads by its model (4 of labels, 4
of the cube) is timed; ``over_copy`` and ``over_measure`` are the ratios to it and to the measure pass.

``--resources`` needs no GPU: registers, LDS, waves per SIMD and scratch of every kernel as the compiler
reports them."""
import argparse
import ctypes
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from exp_link import synthetic_mask, timed      # noqa: E402


def resources():
    from katsdpimager_amd import build
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [build.hipcc()] + build.FLAGS + ['-Rpass-analysis=kernel-resource-usage', '-c',
                                               os.path.join(build.CSRC, 'cube_sources.hip'),
                                               '-o', os.path.join(tmp, 'cube_sources.o')]
        text = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    for block in text.split('Function Name: ')[1:]:
        name = subprocess.run(['c++filt', block.split()[0]], capture_output=True, text=True).stdout.strip()

        def number(key):
            return int(re.search(re.escape(key) + r': (\d+)', block).group(1))
        print(json.dumps(dict(
            kernel=re.sub(r'\(anonymous namespace\)::', '', name).split('(')[0],
            vgprs=number('VGPRs'), sgprs=number('SGPRs'), lds_bytes=number('LDS Size [bytes/block]'),
            waves_per_simd=number('Occupancy [waves/SIMD]'), scratch_bytes=number('ScratchSize [bytes/lane]'))))


def measure(torch, ctx, queue, C, G, one_pixels, repeats):
    from katsdpimager_amd import accel, link, sources
    from katsdpimager_amd._lib import lib, check, SourceLineTable
    stream = queue.stream
    M = G * G
    shape = (C, 1, G, G)
    with torch.cuda.stream(stream):
        gen = torch.Generator(device=ctx.device).manual_seed(1)
        data = torch.randn(shape, generator=gen, device=ctx.device)
        spare = torch.empty(C * M * 8, dtype=torch.uint8, device=ctx.device)
    array = accel.DeviceArray(ctx, shape, np.float32, tensor=data, queue=queue)
    ones = np.ones(C, np.uint8)
    filled = ones.ctypes.data_as(ctypes.c_void_p)
    handle = queue.handle
    base = dict(channels=C, pixels=G, voxels=C * M)

    half = C * M * 4

    def copy():
        with torch.cuda.stream(stream):
            spare[half:2 * half].copy_(spare[:half])
    copy_ms, spread = timed(torch, stream, copy, repeats)
    print(json.dumps(dict(base, case='copy', bytes_per_voxel=8, ms=round(copy_ms, 3), range=spread)), flush=True)

    masks = {}
    with torch.cuda.stream(stream):
        tensor = synthetic_mask(torch, ctx.device, C, G, gen)
        masks['blobs'] = accel.DeviceArray(ctx, shape, np.uint8, tensor=tensor, queue=queue)
        # every voxel of the first one_pixels^2 pixels of every channel: one source
        tensor = torch.zeros(shape, dtype=torch.uint8, device=ctx.device)
        tensor[:, :, :one_pixels, :one_pixels] = 1
        masks['one_source'] = accel.DeviceArray(ctx, shape, np.uint8, queue=queue, tensor=tensor)
    queue.finish()

    params = link.LinkParameters(max_sources=2 ** 21)
    linker = link.LinkTemplate(ctx, params).instantiate(queue, shape)
    tables = (np.ones(C), np.ones(C), np.arange(C, dtype=np.float64), np.ones(C))
    channel_tables = accel.DeviceArray(ctx, (4 * C,), np.float64, queue=queue)
    for name, mask in masks.items():
        labels, catalogue = linker(mask, array, filled=ones)
        N = len(catalogue)
        c0, offsets = sources.ragged(catalogue['c0'], catalogue['c1'])
        total = int(offsets[-1])
        layout = accel.DeviceArray(ctx, (2 * N + 1,), np.int32, queue=queue)
        layout.set(queue, np.concatenate((c0, offsets)))
        c0_ptr, offsets_ptr = layout.ptr, layout.ptr + 4 * N
        sums = accel.DeviceArray(ctx, (total,), np.float64, queue=queue)
        voxels = accel.DeviceArray(ctx, (total,), np.int32, queue=queue)
        finite = accel.DeviceArray(ctx, (total,), np.int32, queue=queue)
        rows = {field: accel.DeviceArray(ctx, (N,), sources.LINE_TABLE_DTYPE[field], queue=queue)
                for field in sources.LINE_TABLE_DTYPE.names}
        struct = SourceLineTable(**{field: a.ptr for field, a in rows.items()})

        def run_spectra():
            check(lib().kimg_cube_source_spectra(labels.ptr, M, array.ptr, M, C, M, filled, N, c0_ptr, offsets_ptr,
                                                 total, sums.ptr, voxels.ptr, finite.ptr, handle), 'spectra')

        def run_measure():
            check(lib().kimg_cube_measure(labels.ptr, M, array.ptr, M, C, 1, G, G, filled,
                                          ctypes.byref(linker._catalogue), params.max_sources,
                                          linker._tables.ptr, handle), 'measure')

        def run_lines():
            check(lib().kimg_source_lines(N, c0_ptr, offsets_ptr, total, sums.ptr, finite.ptr, C,
                                          *(t.ctypes.data_as(ctypes.c_void_p) for t in tables),
                                          channel_tables.ptr, ctypes.byref(struct), handle), 'lines')

        case = dict(base, mask=name, sources=N, entries=total)
        measure_ms, measure_spread = timed(torch, stream, run_measure, repeats)
        spectra_ms, spectra_spread = timed(torch, stream, run_spectra, repeats)
        lines_ms, lines_spread = timed(torch, stream, run_lines, repeats)
        print(json.dumps(dict(case, entry='measure', ms=round(measure_ms, 3), range=measure_spread,
                              over_copy=round(measure_ms / copy_ms, 2))), flush=True)
        print(json.dumps(dict(case, entry='spectra', ms=round(spectra_ms, 3), range=spectra_spread,
                              over_copy=round(spectra_ms / copy_ms, 2),
                              over_measure=round(spectra_ms / measure_ms, 2))), flush=True)
        print(json.dumps(dict(case, entry='lines', ms=round(lines_ms, 3), range=lines_spread)), flush=True)
        # what was timed is what the catalogue says
        got = voxels.get(queue)
        assert int(got.sum()) == int(catalogue['voxels'].sum()), (int(got.sum()), int(catalogue['voxels'].sum()))
        del labels, layout, sums, voxels, finite, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--channels', type=int, default=64)
    ap.add_argument('--pixels', type=int, default=4096)
    ap.add_argument('--one-source-pixels', type=int, default=1024)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--resources', action='store_true')
    args = ap.parse_args()
    if args.resources:
        return resources()
    import torch
    from katsdpimager_amd import accel
    ctx = accel.Context(0)
    queue = ctx.create_command_queue()
    measure(torch, ctx, queue, args.channels, args.pixels, min(args.one_source_pixels, args.pixels), args.repeats)


if __name__ == '__main__':
    main()
