#!/usr/bin/env python3
"""Time of the per-source moment maps (csrc/cube_source_maps.hip, source_maps.SourceMapper) on one MI355X.

    python tools/exp_source_maps.py [--channels 64] [--pixels 4096] [--one-source-pixels 1024] [--repeats 9]
    python tools/exp_source_maps.py --resources

Unit Gaussian noise, one polarization, and the two inputs of ``exp_link.py`` and ``exp_sources.py``: 1 %
set in compact blobs of 4 x 8 x 8 voxels plus 0.1 % isolated voxels, about a million sources, linked on
the device; and every voxel of the first ``--one-source-pixels`` squared pixels of every channel in one
source.  Per input one untimed call, then ``--repeats`` timed ones on the same buffers, device events
around each: the median and the range of ``kimg_cube_source_maps`` (its memset included), of
``kimg_source_maps_finish``, and of ``kimg_cube_source_spectra`` on the same labels and cube.  In the same
run a device-to-device copy of the 8 bytes a voxel that the pass reads by its model (4 of labels, 4 of
the cube) is timed; ``over_copy`` and ``over_spectra`` are the ratios to it and to the spectra pass.  For
the first ten sources the route this replaces is timed too, per source: ``labels.mask(source=k)``,
``MaskCube.apply`` and ``cube.Moments`` over the source's channels.

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
                                               os.path.join(build.CSRC, 'cube_source_maps.hip'),
                                               '-o', os.path.join(tmp, 'cube_source_maps.o')]
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
    from katsdpimager_amd import accel, cube, detect, link, source_maps, sources
    from katsdpimager_amd._lib import lib, check
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
    x = np.arange(C, dtype=np.float64)

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
        tensor = torch.zeros(shape, dtype=torch.uint8, device=ctx.device)
        tensor[:, :, :one_pixels, :one_pixels] = 1
        masks['one_source'] = accel.DeviceArray(ctx, shape, np.uint8, queue=queue, tensor=tensor)
    queue.finish()

    params = link.LinkParameters(max_sources=2 ** 21)
    linker = link.LinkTemplate(ctx, params).instantiate(queue, shape)
    for name, mask in masks.items():
        labels, catalogue = linker(mask, array, filled=ones)
        N = len(catalogue)
        rows, total = source_maps.source_rows(
            *(catalogue[field] for field in ('polarization', 'y0', 'y1', 'x0', 'x1', 'c0', 'c1')), x, 1.0)
        tables = accel.DeviceArray(ctx, (8 * C + 48 * N,), np.uint8, queue=queue)
        tables.set(queue, np.concatenate((x.view(np.uint8), rows.view(np.uint8))))
        x_ptr, rows_ptr = tables.ptr, tables.ptr + 8 * C
        state_bytes = lib().kimg_cube_source_maps_workspace_bytes(total)
        state = accel.DeviceArray(ctx, (state_bytes // 8 + 1,), np.float64, queue=queue)
        out = [accel.DeviceArray(ctx, (total,), np.int32 if k == 5 else np.float32, queue=queue) for k in range(6)]

        c0, offsets = sources.ragged(catalogue['c0'], catalogue['c1'])
        spectra_total = int(offsets[-1])
        layout = accel.DeviceArray(ctx, (2 * N + 1,), np.int32, queue=queue)
        layout.set(queue, np.concatenate((c0, offsets)))
        sums = accel.DeviceArray(ctx, (spectra_total,), np.float64, queue=queue)
        voxels = accel.DeviceArray(ctx, (spectra_total,), np.int32, queue=queue)
        finite = accel.DeviceArray(ctx, (spectra_total,), np.int32, queue=queue)

        def run_maps():
            check(lib().kimg_cube_source_maps(labels.ptr, M, array.ptr, M, C, 1, G, G, filled, x_ptr, N, rows_ptr,
                                              total, state.ptr, state_bytes, handle), 'maps')

        def run_finish():
            check(lib().kimg_source_maps_finish(N, rows_ptr, total, state.ptr, state_bytes, x_ptr, C, 63,
                                                *(t.ptr for t in out), handle), 'finish')

        def run_spectra():
            check(lib().kimg_cube_source_spectra(labels.ptr, M, array.ptr, M, C, M, filled, N, layout.ptr,
                                                 layout.ptr + 4 * N, spectra_total, sums.ptr, voxels.ptr,
                                                 finite.ptr, handle), 'spectra')

        case = dict(base, mask=name, sources=N, entries=total)
        spectra_ms, spectra_spread = timed(torch, stream, run_spectra, repeats)
        maps_ms, maps_spread = timed(torch, stream, run_maps, repeats)
        finish_ms, finish_spread = timed(torch, stream, run_finish, repeats)
        print(json.dumps(dict(case, entry='spectra', ms=round(spectra_ms, 3), range=spectra_spread,
                              over_copy=round(spectra_ms / copy_ms, 2))), flush=True)
        print(json.dumps(dict(case, entry='maps', ms=round(maps_ms, 3), range=maps_spread,
                              over_copy=round(maps_ms / copy_ms, 2),
                              over_spectra=round(maps_ms / spectra_ms, 2))), flush=True)
        print(json.dumps(dict(case, entry='finish', ms=round(finish_ms, 3), range=finish_spread)), flush=True)
        # what was timed is what the catalogue says
        count = out[5].get(queue)
        assert int(count.sum()) == int(catalogue['finite'].sum()), (int(count.sum()), int(catalogue['finite'].sum()))

        # the three passes per source that this replaces, for the first ten sources
        labels.filled = ones
        per_source = []
        for k in range(1, min(N, 10) + 1):
            row = catalogue[k - 1]
            moments = cube.MomentsTemplate(ctx, cube.MomentParameters(
                (0, 1, 2, 8, 9), axis='frequency', channels=(int(row['c0']), int(row['c1']) + 1))).instantiate(
                    queue, shape)
            own = detect.MaskCube.of_cube(queue, shape, np.uint8, ones)
            blanked = accel.DeviceArray(ctx, shape, np.float32, queue=queue)

            def three_passes():
                check(lib().kimg_cube_label_mask(labels.ptr, M, own.ptr, M, C, M, k, handle), 'label_mask')
                check(lib().kimg_cube_mask_apply(array.ptr, M, own.ptr, M, blanked.ptr, M, C, M, filled, 0, handle),
                      'mask_apply')
                moments(blanked, coordinates=x, filled=ones, channel_width=1.0)
            ms, _ = timed(torch, stream, three_passes, 3)
            per_source.append(round(ms, 3))
            del own, blanked
        print(json.dumps(dict(case, entry='three_passes_per_source', ms=per_source,
                              one_pass_over_three=round((maps_ms + finish_ms) / float(np.median(per_source)), 2))),
              flush=True)
        del labels, tables, state, out, layout, sums, voxels, finite


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
