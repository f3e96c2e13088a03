#!/usr/bin/env python3
"""End-to-end example on synthetic data: raw visibilities -> device preprocessing -> HBM-resident
store -> imaging weights, PSF, major/minor cycles -> restored image, all on one MI355X.

    python examples/image_channel.py [--pixels 2048] [--vis 4000000] [--major 3]
    python examples/image_channel.py --uvcontsub 1:6-9      (a 16-channel band; see uvcontsub_band)
    python examples/image_channel.py --phase-shift=-120,60  (a small field around a source; see phase_shift_field)
    python examples/image_channel.py --uv-taper 30,20,30 --uv-range 0,3000  (see uv_taper_channel)
    python examples/image_channel.py --primary-beam 0.3     (see primary_beam_channel)
    python examples/image_channel.py --spectral hanning,2   (a band with a one-channel line; see spectral_line)
    python examples/image_channel.py --statwt 8             (noise that differs between baselines; see statwt_band)
    python examples/image_channel.py --rfiflag              (bursts of interference in a band of noise; see rfiflag_band)
    python examples/image_channel.py --moments              (a band with two line sources into a cube; see moments_band)
    python examples/image_channel.py --moments --imcontsub 1:1-3,5-10  (... with a continuum source, taken out on the cube)
    python examples/image_channel.py --moments --median-contsub        (... taken out by the per-pixel median, told no line ranges)
    python examples/image_channel.py --moments --common-beam  (... every plane restored with its own beam, then all taken to one)
    python examples/image_channel.py --moments --common-beam --measure-noise  (... and the smoothed planes' noise measured)
    python examples/image_channel.py --moments --find-sources  (... and the smooth-and-clip detection mask of the cube, linked into a catalogue and parameterised: flux, peak, centroid, w50; and every source's own moment maps)

It follows the reference's per-channel flow (frontend.py:31-83 preprocess_visibilities,
:465-658 process_channel) with the loaders and FITS output left out: the sky is three point
sources; the restoring beam is fitted to the PSF.
"""
import argparse
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def uvcontsub_band(args):
    """--uvcontsub ORDER[:first-last,...]: a synthetic band of 16 channels with a continuum source
    whose flux slopes across the band and a line source in channels `first` to `last` (default 6-9),
    through ``loader.preprocess_visibilities`` with and without ``continuum=``; prints the dirty
    peak of a line-free channel before and after, and of a line channel after."""
    import synth
    from katsdpimager_amd import accel, continuum, frontend, imaging, loader, parameters, preprocess, weight
    order, _, spans = args.uvcontsub.partition(':')
    ranges = [(int(a), int(b) + 1) for a, b in (span.split('-') for span in (spans or '6-9').split(','))]
    C = 16
    params = continuum.UVContSubParameters(int(order), line_ranges=ranges)
    free = params.mask(C)
    ctx = accel.create_some_context()
    queue = ctx.create_command_queue()
    rows = max(args.vis // C, 1000)
    obs = synth.make_observation(args.pixels, rows, args.w_planes, 1, device='cpu')
    image_p, grid_p, array_p = synth.make_parameters(obs, 1, args.kernel_width, degrid=True)
    uvw = obs.uvw.numpy()
    uvw_wl = uvw.astype(np.float64) / obs.wavelength

    def source(lp, mp):
        l, m = lp * obs.pixel_size, mp * obs.pixel_size
        n = math.sqrt(1 - l * l - m * m)
        return np.exp(-2j * np.pi * (uvw_wl[:, 0] * l + uvw_wl[:, 1] * m + uvw_wl[:, 2] * (n - 1))) / n
    x = continuum.legendre_basis(1, C)[1]
    vis = source(40, -25)[:, None] * (1.0 + 0.3 * x)[None, :]       # 1 Jy at band centre, sloped
    line_pos = (-120, 60)
    vis[:, free == 0] += 0.5 * source(*line_pos)[:, None]
    dataset = loader.LoaderArrays(uvw, vis[:, :, None].astype(np.complex64),
                                  np.ones((rows, C, 1), np.float32), np.zeros(rows, np.int32),
                                  _frequencies(obs, C), [0])
    weight_p = parameters.WeightParameters(weight.WeightType.ROBUST, 0.0)
    clean_p = parameters.CleanParameters(args.minor, 0.1, 0.85, 5.0, 0, 0.01, 0.5, 0.02)
    template = imaging.ImagingTemplate(ctx, array_p, image_p.fixed, weight_p, grid_p.fixed, clean_p)
    imager = template.instantiate(queue, image_p, grid_p, args.vis_block, 0, 1, streams=2)
    imager.ensure_all_bound()
    # only the first peak of each dirty image is wanted: the reference's own two steps, whatever the
    # PSF patch of so short a synthetic track turns out to be
    imager.one_call_major_cycles = False
    ident = np.ones((1, 1), np.complex64)
    line_free, line = int(np.flatnonzero(free)[0]), int(np.flatnonzero(free == 0)[0])
    peaks = {}
    for label, keyword in (('before', None), ('after', params)):
        collector = preprocess.VisibilityCollectorDevice(queue, [image_p] * C, [grid_p] * C, args.vis_block)
        loader.preprocess_visibilities(dataset, collector, 0, C, (ident, None), continuum=keyword)
        if keyword is not None:
            print('uvcontsub {}: {} samples fitted, {} flagged'.format(params, *collector.continuum_counts))
        for channel in (line_free, line):
            stats = frontend.process_channel(collector.reader(), channel, imager, image_p, grid_p, clean_p,
                                             weight_p.weight_type, args.vis_block, 1, True)
            peaks[label, channel] = float(stats['peaks'][0])
    print('line-free channel {:2d}: dirty peak {:.6f} before, {:.2e} after'.format(
        line_free, peaks['before', line_free], peaks['after', line_free]))
    print('line channel      {:2d}: dirty peak {:.6f} before, {:.6f} after (the 0.5 Jy line source)'.format(
        line, peaks['before', line], peaks['after', line]))
    return peaks


def phase_shift_field(args):
    """--phase-shift L,M: the three-source channel through ``loader.preprocess_visibilities`` twice:
    as it is, imaged on the default field, and with ``phase_centre=`` the direction L, M pixels of
    that field from its centre, imaged on a field a quarter as wide around the new centre.  Prints
    the restored peak of the source nearest to (L, M) in both."""
    import copy
    import synth
    from katsdpimager_amd import (accel, beam, frontend, imaging, loader, parameters, phaseshift,
                                  preprocess, weight)
    L, M = (int(x) for x in args.phase_shift.split(','))
    ctx = accel.create_some_context()
    queue = ctx.create_command_queue()
    obs = synth.make_observation(args.pixels, args.vis, args.w_planes, 1, device='cpu')
    small = copy.copy(obs)
    small.pixels = max(args.pixels // 4, 128)
    small.cell_size = obs.wavelength / (obs.pixel_size * small.pixels)      # (the same pixel size)
    centre = (0.0, math.radians(-45.0))
    new_centre = phaseshift.offset_to_radec(centre, L * obs.pixel_size, M * obs.pixel_size)
    sources = [((40, -25), 1.0), ((-120, 60), 0.5), ((15, 200), 0.25)]      # (l, m) in pixels, Jy
    uvw = obs.uvw.numpy()
    uvw_wl = uvw.astype(np.float64) / obs.wavelength
    vis = np.zeros(obs.n_vis, np.complex128)
    for (lp, mp), flux in sources:
        l, m = lp * obs.pixel_size, mp * obs.pixel_size
        n = math.sqrt(1 - l * l - m * m)
        vis += flux / n * np.exp(-2j * np.pi * (uvw_wl[:, 0] * l + uvw_wl[:, 1] * m + uvw_wl[:, 2] * (n - 1)))
    dataset = loader.LoaderArrays(uvw, vis[:, None, None].astype(np.complex64),
                                  np.ones((obs.n_vis, 1, 1), np.float32), np.zeros(obs.n_vis, np.int32),
                                  _frequencies(obs, 1), [0], phase_centre=centre)
    (lp, mp), flux = min(sources, key=lambda s: (s[0][0] - L) ** 2 + (s[0][1] - M) ** 2)
    weight_p = parameters.WeightParameters(weight.WeightType.ROBUST, 0.0)
    clean_p = parameters.CleanParameters(args.minor, 0.1, 0.85, 5.0, 0, 0.01, 0.5, 0.02)
    ident = np.ones((1, 1), np.complex64)
    peaks = {}
    for label, field, keyword, offset in (('unshifted', obs, None, (lp, mp)),
                                          ('shifted', small, new_centre, (lp - L, mp - M))):
        image_p, grid_p, array_p = synth.make_parameters(field, 1, args.kernel_width, degrid=True)
        collector = preprocess.VisibilityCollectorDevice(queue, [image_p], [grid_p], args.vis_block)
        loader.preprocess_visibilities(dataset, collector, 0, 1, (ident, None), phase_centre=keyword)
        template = imaging.ImagingTemplate(ctx, array_p, image_p.fixed, weight_p, grid_p.fixed, clean_p)
        imager = template.instantiate(queue, image_p, grid_p, args.vis_block, 0, args.major, streams=2)
        imager.ensure_all_bound()
        queue.finish()
        t0 = time.perf_counter()
        stats = frontend.process_channel(collector.reader(), 0, imager, image_p, grid_p, clean_p,
                                         weight_p.weight_type, args.vis_block, args.major, True,
                                         fit_beam=True)
        queue.finish()
        t1 = time.perf_counter()
        beam.restore(imager, stats['restoring_beam'])
        restored = imager.get_buffer('dirty')[0]
        G = field.pixels
        # (the new frame's axes are turned against the old ones by the shift times sin(dec): a pixel
        # or two at this distance, hence the box)
        y, x = G // 2 + offset[1], G // 2 + offset[0]
        box = restored[y - 3:y + 4, x - 3:x + 4]
        peaks[label] = float(box.max())
        print('{:9s}: {:4d} x {:4d} pixels around (ra, dec) = ({:.6f}, {:.6f}), imaged in {:.1f} ms; the '
              '{:.2f} Jy source at ({}, {}) px of this field: restored peak {:.3f}'.format(
                  label, G, G, *getattr(collector, 'phase_centre', centre), (t1 - t0) * 1e3, flux,
                  offset[0], offset[1], peaks[label]))
    return peaks


def parse_uv_taper(args):
    """``weight.UVTaperParameters`` of --uv-taper ARCSEC[,ARCSEC,DEG] and --uv-range MIN,MAX (None
    without either)."""
    from katsdpimager_amd import weight
    if not args.uv_taper and not args.uv_range:
        return None
    gaussian, angle, cuts = None, 0.0, {}
    if args.uv_taper:
        parts = [float(x) for x in args.uv_taper.split(',')]
        if len(parts) not in (1, 3):
            raise SystemExit('--uv-taper takes ARCSEC or ARCSEC,ARCSEC,DEG')
        gaussian, angle = (parts[0:2], parts[2]) if len(parts) == 3 else (parts[0], 0.0)
    if args.uv_range:
        low, high = (float(x) for x in args.uv_range.split(','))
        cuts = dict(min_uv=low or None, max_uv=high)
    return weight.UVTaperParameters.from_arcsec(gaussian, angle, **cuts)


def uv_taper_channel(args):
    """--uv-taper / --uv-range: the three-source channel imaged twice from the same resident store,
    robust weighting without and with the taper; prints the fitted restoring beam and the
    normalized noise of both."""
    import torch
    import scipy.optimize       # noqa: F401
    import synth
    from katsdpimager_amd import accel, frontend, imaging, parameters, preprocess, weight
    taper = parse_uv_taper(args)
    ctx = accel.create_some_context()
    queue = ctx.create_command_queue()
    obs = synth.make_observation(args.pixels, args.vis, args.w_planes, 1, device=ctx.device)
    image_p, grid_p, array_p = synth.make_parameters(obs, 1, args.kernel_width, degrid=True)
    sources = [((40, -25), 1.0), ((-120, 60), 0.5), ((15, 200), 0.25)]      # (l, m) in pixels, Jy
    uvw_wl = obs.uvw.to(torch.float64) / obs.wavelength
    vis = torch.zeros(obs.n_vis, dtype=torch.complex128, device=ctx.device)
    for (lp, mp), flux in sources:
        l, m = lp * obs.pixel_size, mp * obs.pixel_size
        n = math.sqrt(1 - l * l - m * m)
        vis += flux / n * torch.exp(-2j * math.pi * (uvw_wl[:, 0] * l + uvw_wl[:, 1] * m + uvw_wl[:, 2] * (n - 1)))
    vis = vis.to(torch.complex64)[None, :, None].contiguous()
    weights = torch.ones((1, obs.n_vis, 1), dtype=torch.float32, device=ctx.device)
    torch.cuda.synchronize()
    collector = preprocess.VisibilityCollectorDevice(queue, [image_p], [grid_p], args.vis_block)
    collector.add(accel.DeviceArray(ctx, (obs.n_vis, 3), np.float32, tensor=obs.uvw),
                  accel.DeviceArray(ctx, weights.shape, np.float32, tensor=weights),
                  accel.DeviceArray(ctx, vis.shape, np.complex64, tensor=vis),
                  None, None, np.ones((1, 1), np.complex64), None)
    collector.close()
    reader = collector.reader()
    clean_p = parameters.CleanParameters(args.minor, 0.1, 0.85, 5.0, 0, 0.01, 0.5, 0.02)
    arcsec = math.degrees(image_p.pixel_size) * 3600.0
    print('pixel {:.3f} arcsec, uv cell {:.2f} wavelengths; {}'.format(arcsec, 1.0 / image_p.image_size, taper))
    results = {}
    for label, keyword in (('untapered', None), ('tapered', taper)):
        weight_p = parameters.WeightParameters(weight.WeightType.ROBUST, 0.0, keyword)
        template = imaging.ImagingTemplate(ctx, array_p, image_p.fixed, weight_p, grid_p.fixed, clean_p)
        imager = template.instantiate(queue, image_p, grid_p, args.vis_block, 0, args.major, streams=2)
        imager.ensure_all_bound()
        stats = frontend.process_channel(reader, 0, imager, image_p, grid_p, clean_p,
                                         weight_p.weight_type, args.vis_block, args.major, True, fit_beam=True)
        beam = stats['restoring_beam']
        results[label] = stats
        print('{:9s}: restoring beam {:.2f} x {:.2f} arcsec ({:.2f} x {:.2f} px) at {:.1f} deg, '
              'normalized_noise {:.4f}, first peak {:.3f}'.format(
                  label, beam.major * arcsec, beam.minor * arcsec, beam.major, beam.minor,
                  math.degrees(beam.theta), stats['normalized_noise'], float(stats['peaks'][0])))
    return results


def primary_beam_channel(args):
    """--primary-beam FWHM_DEG[,CUTOFF]: the three-source channel as an antenna with a cosine-taper
    beam of that width would see it -- every source attenuated by the beam power at its place --
    imaged twice from the same resident store, without and with ``primary_beam=``; prints the
    restored flux of every source before and after the correction next to its true value.  With
    --output the corrected image and the beam are written."""
    import torch
    import scipy.optimize       # noqa: F401
    import synth
    from katsdpimager_amd import accel, beam, frontend, imaging, parameters, preprocess, primary_beam, weight
    fwhm_deg, _, cutoff = args.primary_beam.partition(',')
    fwhm = math.sin(math.radians(float(fwhm_deg)))
    ctx = accel.create_some_context()
    queue = ctx.create_command_queue()
    obs = synth.make_observation(args.pixels, args.vis, args.w_planes, 1, device=ctx.device)
    image_p, grid_p, array_p = synth.make_parameters(obs, 1, args.kernel_width, degrid=True)
    frequency = primary_beam.SPEED_OF_LIGHT / image_p.wavelength
    corner = math.sqrt(0.5) * image_p.image_size
    model = primary_beam.RadialBeam.cosine_taper(
        fwhm, frequency, [0.9 * frequency, 1.1 * frequency], fwhm / 256.0, min(corner, 2.0 * fwhm))
    params = primary_beam.PrimaryBeamParameters(model, float(cutoff) if cutoff else 0.1)
    G = args.pixels
    lm_scale, lm_bias = image_p.pixel_size, -0.5 * G * image_p.pixel_size
    sources = [((40, -25), 1.0), ((-120, 60), 0.5), ((15, 200), 0.25)]      # (l, m) in pixels, Jy
    # the beam on the pixel grid, as the device samples it
    beam_image = primary_beam.sample_host(model.row(frequency), model.step, G, G, lm_scale, lm_bias)
    uvw_wl = obs.uvw.to(torch.float64) / obs.wavelength
    vis = torch.zeros(obs.n_vis, dtype=torch.complex128, device=ctx.device)
    for (lp, mp), flux in sources:
        l, m = lp * obs.pixel_size, mp * obs.pixel_size
        n = math.sqrt(1 - l * l - m * m)
        power = float(beam_image[G // 2 + mp, G // 2 + lp])
        vis += flux * power / n * torch.exp(
            -2j * math.pi * (uvw_wl[:, 0] * l + uvw_wl[:, 1] * m + uvw_wl[:, 2] * (n - 1)))
    vis = vis.to(torch.complex64)[None, :, None].contiguous()
    weights = torch.ones((1, obs.n_vis, 1), dtype=torch.float32, device=ctx.device)
    torch.cuda.synchronize()
    collector = preprocess.VisibilityCollectorDevice(queue, [image_p], [grid_p], args.vis_block)
    collector.add(accel.DeviceArray(ctx, (obs.n_vis, 3), np.float32, tensor=obs.uvw),
                  accel.DeviceArray(ctx, weights.shape, np.float32, tensor=weights),
                  accel.DeviceArray(ctx, vis.shape, np.complex64, tensor=vis),
                  None, None, np.ones((1, 1), np.complex64), None)
    collector.close()
    reader = collector.reader()
    weight_p = parameters.WeightParameters(weight.WeightType.ROBUST, 0.0)
    clean_p = parameters.CleanParameters(args.minor, 0.1, 0.85, 5.0, 0, 0.01, 0.5, 0.02)
    template = imaging.ImagingTemplate(ctx, array_p, image_p.fixed, weight_p, grid_p.fixed, clean_p)
    imager = template.instantiate(queue, image_p, grid_p, args.vis_block, 0, args.major, streams=2)
    imager.ensure_all_bound()
    print('field {:.3f} deg across, beam FWHM {:.3f} deg at {:.1f} MHz, cutoff {}'.format(
        math.degrees(image_p.image_size), float(fwhm_deg), frequency / 1e6, params.cutoff))
    peaks = {}
    for label, keyword in (('before', None), ('after', params)):
        stats = frontend.process_channel(reader, 0, imager, image_p, grid_p, clean_p,
                                         weight_p.weight_type, args.vis_block, args.major, True,
                                         fit_beam=True, primary_beam=keyword)
        beam.restore(imager, stats['restoring_beam'])
        restored = imager.get_buffer('dirty')
        for (lp, mp), flux in sources:
            y, x = G // 2 + mp, G // 2 + lp
            peaks[label, lp, mp] = float(np.nanmax(restored[0, y - 3:y + 4, x - 3:x + 4]))
    print('pixels kept (beam power >= {}): {} of {}'.format(params.cutoff, stats['beam_valid'], G * G))
    for (lp, mp), flux in sources:
        print('source at (l, m) = ({:5d}, {:5d}) px, true {:.2f} Jy, beam power {:.3f}: restored peak '
              '{:.3f} before, {:.3f} after the correction'.format(
                  lp, mp, flux, float(beam_image[G // 2 + mp, G // 2 + lp]), peaks['before', lp, mp],
                  peaks['after', lp, mp]))
    if args.output:
        from katsdpimager_amd import io, polarization
        image_p.fixed.polarizations = [polarization.STOKES_I]
        centre = (0.0, math.radians(-45.0))
        io.write_fits_image(restored, image_p, args.output, 0, centre, beam=stats['restoring_beam'])
        beam_name = os.path.splitext(args.output)[0] + '_primary_beam.fits'
        io.write_fits_image(stats['beam_power'].get(queue)[np.newaxis], image_p, beam_name, 0, centre,
                            bunit='')
        print('wrote', args.output, 'and', beam_name)
    return peaks


def spectral_line(args):
    """--spectral hanning[,N]: a synthetic band of 8 N channels with a 1 Jy line source in ONE input
    channel, through ``loader.preprocess_visibilities`` without and with ``spectral=`` Hanning
    smoothing (then N channels averaged to one); prints the dirty peak of the line in every output
    channel it reaches next to the share of the input the filter's coefficients predict (1/4, 1/2, 1/4
    for plain Hanning), and checks that the other output channels are empty."""
    import synth
    from katsdpimager_amd import accel, frontend, imaging, loader, parameters, preprocess, spectral, weight
    name, _, n = args.spectral.partition(',')
    if name != 'hanning':
        raise SystemExit('--spectral takes hanning or hanning,N')
    params = spectral.SpectralParameters.hanning(bin=int(n) if n else 1)
    C = 8 * params.bin
    C_out = params.output_channels(C)
    line_channel = 4 * params.bin
    g, offset, step = params.coefficients()
    expected = np.zeros(C_out)
    for o in range(C_out):
        i = line_channel - (o * step - offset)
        if 0 <= i < len(g):
            expected[o] = g[i] / g.sum()
    ctx = accel.create_some_context()
    queue = ctx.create_command_queue()
    rows = max(args.vis // C, 1000)
    obs = synth.make_observation(args.pixels, rows, args.w_planes, 1, device='cpu')
    image_p, grid_p, array_p = synth.make_parameters(obs, 1, args.kernel_width, degrid=True)
    uvw = obs.uvw.numpy()
    uvw_wl = uvw.astype(np.float64) / obs.wavelength
    l, m = 40 * obs.pixel_size, -25 * obs.pixel_size
    nn = math.sqrt(1 - l * l - m * m)
    vis = np.zeros((rows, C, 1), np.complex64)
    vis[:, line_channel, 0] = np.exp(
        -2j * np.pi * (uvw_wl[:, 0] * l + uvw_wl[:, 1] * m + uvw_wl[:, 2] * (nn - 1))) / nn
    dataset = loader.LoaderArrays(uvw, vis, np.ones((rows, C, 1), np.float32), np.zeros(rows, np.int32),
                                  _frequencies(obs, C), [0])
    weight_p = parameters.WeightParameters(weight.WeightType.ROBUST, 0.0)
    clean_p = parameters.CleanParameters(args.minor, 0.1, 0.85, 5.0, 0, 0.01, 0.5, 0.02)
    template = imaging.ImagingTemplate(ctx, array_p, image_p.fixed, weight_p, grid_p.fixed, clean_p)
    imager = template.instantiate(queue, image_p, grid_p, args.vis_block, 0, 1, streams=2)
    imager.ensure_all_bound()
    imager.one_call_major_cycles = False        # (only the first peak of each dirty image is wanted)
    ident = np.ones((1, 1), np.complex64)

    def dirty_peak(collector, channel):
        stats = frontend.process_channel(collector.reader(), channel, imager, image_p, grid_p, clean_p,
                                         weight_p.weight_type, args.vis_block, 1, True)
        return float(stats['peaks'][0])
    raw = preprocess.VisibilityCollectorDevice(queue, [image_p] * C, [grid_p] * C, args.vis_block)
    loader.preprocess_visibilities(dataset, raw, 0, C, (ident, None))
    peak_in = dirty_peak(raw, line_channel)
    filtered = preprocess.VisibilityCollectorDevice(queue, [image_p] * C_out, [grid_p] * C_out, args.vis_block)
    loader.preprocess_visibilities(dataset, filtered, 0, C, (ident, None), spectral=params)
    print('{}: {} channels to {}; {} output samples kept, {} flagged'.format(
        params, C, C_out, *filtered.spectral_counts))
    print('input channel {:2d}: dirty peak {:.6f}'.format(line_channel, peak_in))
    reader = filtered.reader()
    peaks = {'input': peak_in}
    for o in range(C_out):
        if expected[o] > 0:
            peaks[o] = dirty_peak(filtered, o)
            print('output channel {:2d}: dirty peak {:.6f} = {:.6f} of the input (coefficients: {:.6f})'.format(
                o, peaks[o], peaks[o] / peak_in, expected[o]))
        else:
            largest = max((float(np.abs(piece['vis']).max()) for s in range(reader.num_w_slices(o))
                           for piece in reader.iter_slice(o, s, None)), default=0.0)
            peaks[o] = largest
            print('output channel {:2d}: largest |vis| {:g}'.format(o, largest))
    peaks['expected'] = expected
    return peaks


def statwt_band(args):
    """--statwt TIME_BIN[:first-last,...]: a synthetic band of 16 channels of pure noise whose sigma
    differs from baseline to baseline (0.5 to 4) while every weight is 1, through
    ``loader.preprocess_visibilities`` without and with ``statwt=`` (the listed channels left out of
    the statistic); prints, for one channel, the image noise the weights predict (``weights_noise``),
    ``normalized_noise`` and the rms measured in the central half of the dirty image (robust
    weighting).  With weights that are inverse variances the prediction is the measurement."""
    import synth
    from katsdpimager_amd import accel, frontend, imaging, loader, parameters, preprocess, statwt, weight
    time_bin, _, spans = args.statwt.partition(':')
    ranges = [(int(a), int(b) + 1) for a, b in (span.split('-') for span in spans.split(','))] if spans else None
    C = 16
    params = statwt.StatWtParameters(int(time_bin), line_ranges=ranges)
    ctx = accel.create_some_context()
    queue = ctx.create_command_queue()
    rows = max(args.vis // C, 1000)
    obs = synth.make_observation(args.pixels, rows, args.w_planes, 1, device='cpu')
    image_p, grid_p, array_p = synth.make_parameters(obs, 1, args.kernel_width, degrid=True)
    # (synth's tracks are baseline-major: ceil(rows / baselines) consecutive rows each)
    num_baselines = synth.baselines_equatorial().shape[0]
    baseline = (np.arange(rows) // -(-rows // num_baselines)).astype(np.int32)
    rng = np.random.default_rng(5)
    sigma = rng.uniform(0.5, 4.0, num_baselines)[baseline]
    vis = ((rng.normal(size=(rows, C, 1)) + 1j * rng.normal(size=(rows, C, 1)))
           * sigma[:, None, None]).astype(np.complex64)
    dataset = loader.LoaderArrays(obs.uvw.numpy(), vis, np.ones((rows, C, 1), np.float32), baseline,
                                  _frequencies(obs, C), [0])
    weight_p = parameters.WeightParameters(weight.WeightType.ROBUST, 0.0)
    # (one minor cycle: the residual is the dirty image but for one component of noise)
    clean_p = parameters.CleanParameters(1, 0.1, 0.85, 5.0, 0, 0.01, 0.5, 0.02)
    template = imaging.ImagingTemplate(ctx, array_p, image_p.fixed, weight_p, grid_p.fixed, clean_p)
    imager = template.instantiate(queue, image_p, grid_p, args.vis_block, 0, 1, streams=2)
    imager.ensure_all_bound()
    imager.one_call_major_cycles = False
    ident = np.ones((1, 1), np.complex64)
    channel = int(np.flatnonzero(params.mask(C))[0])
    G = args.pixels
    results = {}
    print('{} rows of {} channels, {} baselines with sigma 0.5 to 4, every weight 1; channel {}'.format(
        rows, C, len(np.unique(baseline)), channel))
    for label, keyword in (('weights as given', None), ('reweighted', params)):
        collector = preprocess.VisibilityCollectorDevice(queue, [image_p] * C, [grid_p] * C, args.vis_block)
        loader.preprocess_visibilities(dataset, collector, 0, C, (ident, None), statwt=keyword)
        if keyword is not None:
            print('statwt {}: {} groups kept, {} flagged'.format(params, *collector.statwt_counts))
        reader = collector.reader()
        stats = frontend.process_channel(reader, channel, imager, image_p, grid_p, clean_p,
                                         weight_p.weight_type, args.vis_block, 1, True)
        dirty = imager.get_buffer('dirty')[0][G // 4:3 * G // 4, G // 4:3 * G // 4]
        rms = float(np.sqrt(np.mean(np.square(dirty, dtype=np.float64))))
        results[label] = dict(weights_noise=stats['weights_noise'], normalized_noise=stats['normalized_noise'],
                              rms=rms)
        print('{:16s}: weights predict an image noise of {:.6g}, normalized_noise {:.4f}; measured rms '
              '{:.6g}, {:.3f} of the prediction'.format(
                  label, stats['weights_noise'], stats['normalized_noise'], rms,
                  rms / stats['weights_noise']))
    return results


def rfiflag_band(args):
    """--rfiflag [THRESHOLD]: a synthetic band of 16 channels of noise of sigma 1 under weights of
    1 with bursts of interference injected -- one channel x 5 integrations of 30 sigma on every 50th
    baseline, one integration x all channels of 10 sigma on every 50th other -- through
    ``loader.preprocess_visibilities`` with ``statwt=`` (groups of 8 rows), without and with
    ``rfiflag=``; prints, for one channel, the fraction of samples flagged, the image noise statwt's
    weights predict and the rms measured in the central half of the dirty image."""
    import synth
    from katsdpimager_amd import (accel, frontend, imaging, loader, parameters, preprocess, rfiflag, statwt,
                                  weight)
    keywords = dict(threshold=float(args.rfiflag)) if args.rfiflag else {}
    C = 16
    params = rfiflag.RFIFlagParameters(**keywords)
    reweight = statwt.StatWtParameters(8)
    ctx = accel.create_some_context()
    queue = ctx.create_command_queue()
    rows = max(args.vis // C, 1000)
    obs = synth.make_observation(args.pixels, rows, args.w_planes, 1, device='cpu')
    image_p, grid_p, array_p = synth.make_parameters(obs, 1, args.kernel_width, degrid=True)
    # (synth's tracks are baseline-major: ceil(rows / baselines) consecutive rows each)
    num_baselines = synth.baselines_equatorial().shape[0]
    per_baseline = -(-rows // num_baselines)
    baseline = (np.arange(rows) // per_baseline).astype(np.int32)
    rng = np.random.default_rng(6)
    vis = (rng.normal(size=(rows, C, 1)) + 1j * rng.normal(size=(rows, C, 1))).astype(np.complex64)
    bursts = 0
    for b in range(0, int(baseline[-1]) + 1, 25):
        first = b * per_baseline + int(rng.integers(max(per_baseline - 5, 1)))
        if b % 50 == 0:
            vis[first:first + 5, int(rng.integers(C)), 0] += np.complex64(30.0)
        else:
            vis[first, :, 0] += np.complex64(10.0)
        bursts += 1
    dataset = loader.LoaderArrays(obs.uvw.numpy(), vis, np.ones((rows, C, 1), np.float32), baseline,
                                  _frequencies(obs, C), [0])
    weight_p = parameters.WeightParameters(weight.WeightType.ROBUST, 0.0)
    # (one minor cycle: the residual is the dirty image but for one component of noise)
    clean_p = parameters.CleanParameters(1, 0.1, 0.85, 5.0, 0, 0.01, 0.5, 0.02)
    template = imaging.ImagingTemplate(ctx, array_p, image_p.fixed, weight_p, grid_p.fixed, clean_p)
    imager = template.instantiate(queue, image_p, grid_p, args.vis_block, 0, 1, streams=2)
    imager.ensure_all_bound()
    imager.one_call_major_cycles = False
    ident = np.ones((1, 1), np.complex64)
    G = args.pixels
    results = {}
    print('{} rows of {} channels, {} baselines of {} rows, noise of sigma 1, {} bursts'.format(
        rows, C, len(np.unique(baseline)), per_baseline, bursts))
    for label, keyword in (('not flagged', None), ('flagged', params)):
        collector = preprocess.VisibilityCollectorDevice(queue, [image_p] * C, [grid_p] * C, args.vis_block)
        loader.preprocess_visibilities(dataset, collector, 0, C, (ident, None), statwt=reweight,
                                       rfiflag=keyword)
        fraction = 0.0
        if keyword is not None:
            kept, flagged, skipped = collector.rfiflag_counts
            fraction = flagged / max(kept + flagged, 1)
            print('rfiflag {}: {} samples kept, {} flagged, {} pairs skipped'.format(params, kept, flagged, skipped))
        reader = collector.reader()
        stats = frontend.process_channel(reader, 0, imager, image_p, grid_p, clean_p,
                                         weight_p.weight_type, args.vis_block, 1, True)
        dirty = imager.get_buffer('dirty')[0][G // 4:3 * G // 4, G // 4:3 * G // 4]
        rms = float(np.sqrt(np.mean(np.square(dirty, dtype=np.float64))))
        results[label] = dict(flagged_fraction=fraction, weights_noise=stats['weights_noise'], rms=rms)
        print('{:12s}: {:.4f} of the samples flagged; statwt\'s weights predict an image noise of {:.6g}; '
              'measured rms {:.6g}'.format(label, fraction, stats['weights_noise'], rms))
    return results


def moments_band(args):
    """--moments: a synthetic band of 12 channels with two line sources -- A at (40, -25) px with a
    line three channels wide about channel 2, B at (-60, -200) px with a line about channel 7.5 and
    twice as wide: the line centre moves across the field.  (With one major cycle the minor cycles
    take out only the PSF patch around a component, so far from a source the residual still holds
    its dirty sidelobes.  At 512 px the PSF of this array is -0.0008 at the offset between A and B:
    the other source's channels stay under the cut.  At (-120, 60) px it is +0.014, above three of
    the robust noise estimates of 0.0043 per Jy, and they would enter the sums.)  Every channel that holds emission is
    imaged and CLEANed (one major cycle), the model is added back to the residual, and the image
    goes into a :class:`cube.SpectralCube` with the channel's noise estimate; the other channels stay
    unfilled.  The cube lives on a queue of its own: ``put`` waits for the imager's queue and the
    imager waits for the copy.  Prints moments 0, 1 and 2 (``clip_sigma=3``, radio velocity about the
    band centre) at the two positions next to what was injected; ``--output`` writes the cube.

    With ``--imcontsub ORDER[:first-last,...]`` a continuum source of 0.4 Jy, sloping by 0.01 Jy a
    channel, lies on source A, so every channel is imaged; moment 0 is taken twice, of the cube as
    imaged and after ``imcontsub.ImContSub`` has fitted a polynomial of that order per pixel to the
    channels outside the listed ranges (default 1-3,5-10, the two lines) and subtracted it in place,
    and both are printed next to the injected line integral.

    With ``--common-beam`` every channel's beam is fitted to its PSF and the plane is restored with
    it (the model convolved with the beam, plus the residual) and ``put`` with it; the moments are
    taken twice, of the cube as imaged and of the cube ``smooth.CubeSmooth`` has taken to the common
    beam, and every plane's fitted beam, the common beam and moment 0 at source A without and with
    the smoothing are printed.  The smoothed planes' noise is the unsmoothed one times the flux factor, a
    stand-in; with ``--measure-noise`` ``cube_stats.CubeStats`` measures it on the smoothed cube, both
    are printed per channel and the measured one makes the ``clip_sigma`` cuts."""
    import synth
    from katsdpimager_amd import (accel, beam, cube, cube_stats, frontend, imaging, imcontsub, loader,
                                  parameters, preprocess, smooth, weight)
    C = 12
    contsub = None
    if args.imcontsub:
        order, _, spans = args.imcontsub.partition(':')
        ranges = [(int(a), int(b) + 1) for a, b in (span.split('-') for span in (spans or '1-3,5-10').split(','))]
        contsub = imcontsub.ImContSubParameters(int(order), line_ranges=ranges)
        contsub.mask(C)
    line_a = np.zeros(C)
    line_a[1:4] = [0.5, 1.0, 0.5]
    line_b = np.zeros(C)
    line_b[5:11] = [0.3, 0.6, 0.9, 0.9, 0.6, 0.3]
    positions = {'A': (40, -25), 'B': (-60, -200)}
    lines = {'A': line_a, 'B': line_b}
    ctx = accel.create_some_context()
    queue = ctx.create_command_queue()
    cube_queue = ctx.create_command_queue()
    rows = max(args.vis // C, 1000)
    obs = synth.make_observation(args.pixels, rows, args.w_planes, 1, device='cpu')
    image_p, grid_p, array_p = synth.make_parameters(obs, 1, args.kernel_width, degrid=True)
    uvw = obs.uvw.numpy()
    uvw_wl = uvw.astype(np.float64) / obs.wavelength
    vis = np.zeros((rows, C), np.complex128)
    for name, (lp, mp) in positions.items():
        l, m = lp * obs.pixel_size, mp * obs.pixel_size
        n = math.sqrt(1 - l * l - m * m)
        source = np.exp(-2j * np.pi * (uvw_wl[:, 0] * l + uvw_wl[:, 1] * m + uvw_wl[:, 2] * (n - 1))) / n
        vis += source[:, None] * lines[name][None, :]
        if (contsub is not None or args.median_contsub) and name == 'A':
            vis += source[:, None] * (0.4 + 0.01 * (np.arange(C) - 5.5))[None, :]
    frequencies = _frequencies(obs, C)
    rest_frequency = float(frequencies[C // 2])
    dataset = loader.LoaderArrays(uvw, vis[:, :, None].astype(np.complex64),
                                  np.ones((rows, C, 1), np.float32), np.zeros(rows, np.int32),
                                  frequencies, [0])
    weight_p = parameters.WeightParameters(weight.WeightType.ROBUST, 0.0)
    clean_p = parameters.CleanParameters(args.minor, 0.1, 0.85, 5.0, 0, 0.01, 0.5, 0.02)
    template = imaging.ImagingTemplate(ctx, array_p, image_p.fixed, weight_p, grid_p.fixed, clean_p)
    imager = template.instantiate(queue, image_p, grid_p, args.vis_block, 0, 1, streams=2)
    imager.ensure_all_bound()
    collector = preprocess.VisibilityCollectorDevice(queue, [image_p] * C, [grid_p] * C, args.vis_block)
    loader.preprocess_visibilities(dataset, collector, 0, C, (np.ones((1, 1), np.complex64), None))
    G = args.pixels
    sc = cube.SpectralCube(ctx, cube_queue, frequencies, [0], (G, G), channel_width=frequencies[1] - frequencies[0])
    restorer = None
    for channel in range(C):
        if contsub is None and not args.median_contsub and line_a[channel] == 0 and line_b[channel] == 0:
            continue
        stats = frontend.process_channel(collector.reader(), channel, imager, image_p, grid_p, clean_p,
                                         weight_p.weight_type, args.vis_block, 1, True,
                                         fit_beam=args.common_beam)
        if stats is None:
            continue
        fitted = stats.get('restoring_beam')
        if fitted is not None:
            restorer = beam.restore(imager, fitted, restorer)
        else:
            imager.add_model_to_dirty()
        copied = sc.put(channel, imager.buffer('dirty'), stats['noise'], wait_for=[queue.enqueue_marker()],
                        beam=fitted)
        queue.enqueue_wait_for_events([copied])         # (the next channel rewrites the buffer)
    params = cube.MomentParameters((0, 1, 2), rest_frequency=rest_frequency, clip_sigma=3.0)
    moments = cube.MomentsTemplate(ctx, params).instantiate(cube_queue, sc.shape)
    unsubtracted = continuum_map = None
    if contsub is not None:
        unsubtracted = moments(sc)[0].get(cube_queue)[0]
        fit = imcontsub.ImContSubTemplate(ctx, contsub).instantiate(cube_queue, sc.shape)(sc)
        continuum_map = fit['continuum'].get(cube_queue)[0]
        print('imcontsub {}: {} of {} pixels fitted'.format(
            contsub, int((fit['count'].get(cube_queue) >= contsub.order + 1).sum()), G * G))
    median_contsub = None
    if args.median_contsub:
        # the continuum of source A three ways: left in, taken out by a first-order fit that is told
        # where the lines are (--imcontsub 1), and by the per-pixel median that is told nothing
        from katsdpimager_amd import spectrum_stats
        y, x = G // 2 + positions['A'][1], G // 2 + positions['A'][0]
        left_in = float(moments(sc)[0].get(cube_queue)[0][y, x])
        copies = [cube.SpectralCube(ctx, cube_queue, frequencies, [0], (G, G), channel_width=sc.channel_width)
                  for _ in range(2)]
        told = imcontsub.ImContSubParameters(1, line_ranges=[(1, 4), (5, 11)])
        imcontsub.ImContSubTemplate(ctx, told).instantiate(cube_queue, sc.shape)(sc, out=copies[0])
        median_op = spectrum_stats.SpectrumStatsTemplate(
            ctx, spectrum_stats.SpectrumStatsParameters()).instantiate(cube_queue, sc.shape)
        median_maps = median_op(sc, subtract=True, out=copies[1])
        fitted = float(moments(copies[0])[0].get(cube_queue)[0][y, x])
        sc = copies[1]
        by_median = float(moments(sc)[0].get(cube_queue)[0][y, x])
        median_contsub = dict(left_in=left_in, imcontsub=fitted, median=by_median,
                              continuum=float(median_maps['median'].get(cube_queue)[0][y, x]),
                              sigma=float(median_maps['sigma'].get(cube_queue)[0][y, x]))
    unsmoothed = None
    if args.common_beam:
        y, x = G // 2 + positions['A'][1], G // 2 + positions['A'][0]
        unsmoothed = float(moments(sc)[0].get(cube_queue)[0][y, x])
        smoother = smooth.CubeSmoothTemplate(ctx, smooth.CommonBeamParameters()).instantiate(cube_queue, sc.shape)
        smoothed = smoother(sc)
        for channel in np.flatnonzero(sc.filled):
            print('channel {:2d}: beam {!r}, kernel radius {}, flux factor {:.6f}'.format(
                int(channel), sc.beams[channel], int(smoother.radius[channel]),
                float(smoother.factors[channel])))
        print('common beam {!r}'.format(smoothed.common_beam))
        # (the noise of a smoothed plane is the caller's to set: here the input's, scaled)
        smoothed.noise[:] = sc.noise * smoother.factors.astype(np.float32)
        if args.measure_noise:
            # ... or measured: the stand-in is the unsmoothed noise times the flux factor, and the
            # noise of a smoothed plane is correlated and differs from it
            stand_in = smoothed.noise.copy()
            measure = cube_stats.CubeStatsTemplate(ctx, cube_stats.CubeStatsParameters()).instantiate(
                cube_queue, smoothed.shape)
            measured = measure(smoothed, update_noise=True)
            for channel in np.flatnonzero(smoothed.filled):
                print('channel {:2d}: noise {:.4e} as scaled, {:.4e} measured on the smoothed plane '
                      '({} samples)'.format(int(channel), float(stand_in[channel]),
                                            float(smoothed.noise[channel]), int(measured.count[channel, 0])))
        sc = smoothed
    maps = moments(sc)
    host = {key: value.get(cube_queue)[0] for key, value in maps.items()}
    if unsmoothed is not None:
        print('moment 0 at source A: {:12.6f} without the smoothing, {:12.6f} with it'.format(
            unsmoothed, float(host[0][y, x])))
    velocity = sc.coordinates('velocity', rest_frequency)
    width = abs(velocity[-1] - velocity[0]) / (C - 1)
    print('{} channels of {:.1f} km/s, {} imaged; noise estimates {:.2e} to {:.2e}'.format(
        C, width, int(sc.filled.sum()), float(np.nanmin(sc.noise)), float(np.nanmax(sc.noise))))
    results = dict(noise=sc.noise.copy(), filled=sc.filled.copy(), width=width, velocity=velocity, sources={})
    for name, (lp, mp) in positions.items():
        y, x = G // 2 + mp, G // 2 + lp
        line = lines[name]
        centre = float((line * velocity).sum() / line.sum())
        injected = (float(line.sum() * width), centre,
                    float(np.sqrt((line * (velocity - centre) ** 2).sum() / line.sum())))
        got = tuple(float(host[m][y, x]) for m in (0, 1, 2))
        results['sources'][name] = dict(injected=injected, moments=got, count=int(host['count'][y, x]))
        print('source {} at (l, m) = ({:5d}, {:5d}) px, {} samples entered:'.format(
            name, lp, mp, int(host['count'][y, x])))
        for m, unit in ((0, 'Jy/beam.km/s'), (1, 'km/s'), (2, 'km/s')):
            print('  moment {}: {:12.6f} {}, injected {:12.6f}'.format(m, got[m], unit, injected[m]))
        if contsub is not None:
            results['sources'][name].update(unsubtracted=float(unsubtracted[y, x]),
                                            continuum=float(continuum_map[y, x]))
            print('  moment 0 without the subtraction: {:12.6f}; continuum map {:.4f} Jy/beam'.format(
                float(unsubtracted[y, x]), float(continuum_map[y, x])))
    if median_contsub is not None:
        results['median_contsub'] = median_contsub
        print('moment 0 at source A, injected {:.6f}: {:.6f} with the continuum left in, {:.6f} after '
              '--imcontsub 1, {:.6f} after the median subtraction (median map {:.4f} Jy/beam, sigma map '
              '{:.2e})'.format(results['sources']['A']['injected'][0], median_contsub['left_in'],
                               median_contsub['imcontsub'], median_contsub['median'],
                               median_contsub['continuum'], median_contsub['sigma']))
    if args.find_sources:
        # moment 0 at the first line source three ways: everything finite, the per-voxel 3 sigma clip
        # (above), and through the smooth-and-clip mask, which measures every smoothed copy's noise itself
        from katsdpimager_amd import detect
        name = next(iter(positions))
        y, x = G // 2 + positions[name][1], G // 2 + positions[name][0]
        finder = detect.SmoothClipTemplate(ctx, detect.SmoothClipParameters()).instantiate(cube_queue, sc.shape)
        found = finder(sc)
        voxels = int(found.get(cube_queue).sum())
        plain = cube.MomentsTemplate(ctx, cube.MomentParameters((0,), rest_frequency=rest_frequency)).instantiate(
            cube_queue, sc.shape)
        unclipped = float(plain(sc)[0].get(cube_queue)[0][y, x])
        through = float(plain(found.apply(sc))[0].get(cube_queue)[0][y, x])
        results['find_sources'] = dict(voxels=voxels, unclipped=unclipped, through_mask=through,
                                       clipped=results['sources'][name]['moments'][0])
        print('smooth-and-clip at {} sigma: {} of {} voxels detected'.format(
            finder.params.threshold, voxels, int(np.prod(sc.shape))))
        print('moment 0 at source {}, injected {:.6f}: {:.6f} unclipped, {:.6f} with clip_sigma=3, '
              '{:.6f} through the mask'.format(name, results['sources'][name]['injected'][0], unclipped,
                                               results['sources'][name]['moments'][0], through))
        # the mask linked into sources: the catalogue, and moment 0 of the first source through its own mask
        from katsdpimager_amd import link
        linker = link.LinkTemplate(ctx, link.LinkParameters(radius_xy=1.5, min_voxels=3)).instantiate(
            cube_queue, sc.shape)
        labels, catalogue = linker(found, sc)
        results['find_sources']['catalogue'] = [
            {field: row[field].tolist() for field in catalogue.dtype.names} for row in catalogue]
        print('{} sources of at least 3 voxels:'.format(len(catalogue)))
        for row in catalogue:
            print('  {:3d}: {:5d} voxels, peak {:.6f} at (c, y, x) = ({}, {}, {}), sum {:.6f}, centroid '
                  '({:.2f}, {:.2f}, {:.2f}), {:.6f} MHz'.format(
                      row['id'], row['voxels'], row['peak'], row['peak_c'], row['peak_y'], row['peak_x'],
                      row['sum'], *row['centroid'], row['frequency'] / 1e6))
        if len(catalogue):
            own = plain(labels.mask(source=1).apply(sc))[0].get(cube_queue)[0]
            results['find_sources']['first_source_moment0'] = float(np.nansum(own))
            print('moment 0 of source 1 through its own mask: {} pixels, {:.6f} in all'.format(
                int(np.isfinite(own).sum()), float(np.nansum(own))))
            # every source's spectrum in one more pass, and what a parameteriser makes of it: in Jy
            # where the planes carry their beams (--common-beam), else in sums of pixel values
            from katsdpimager_amd import sources
            with_beams = sc.common_beam is not None or all(
                sc.beams[c] is not None for c in np.flatnonzero(sc.filled))
            source_params = sources.SourceParameters(rest_frequency=rest_frequency,
                                                     units='beam' if with_beams else 'pixel')
            parameteriser = sources.SourcesTemplate(ctx, source_params).instantiate(cube_queue, sc.shape)
            spectra, source_lines = parameteriser(labels, sc, catalogue)
            first = source_lines[0]
            unit = 'Jy' if with_beams else 'Jy/beam.pixel'
            results['find_sources'].update(
                flux_unit=unit + '.km/s', first_source_flux=float(first['flux']),
                first_source_flux_err=float(first['flux_err']), first_source_peak=float(first['peak']),
                first_source_centroid=float(first['centroid']), first_source_w50=float(first['w50']),
                first_source_w20=float(first['w20']),
                first_source_spectrum=[t.tolist() for t in spectra.spectrum(1)])
            line = lines[name]
            print('source 1 from its spectrum ({} channels): flux {:.6f} +- {:.6f} {}.km/s, peak {:.6f} {} in '
                  'channel {}, centroid {:.3f} km/s, w50 {:.3f} km/s, w20 {:.3f} km/s; the line injected at '
                  'source {} has its centroid at {:.3f} km/s and {:.3f} km/s above half its peak'.format(
                      int(first['channels']), first['flux'], first['flux_err'], unit, first['peak'], unit,
                      int(first['peak_channel']), first['centroid'], first['w50'], first['w20'], name,
                      results['sources'][name]['injected'][1],
                      float(np.ptp(velocity[line >= 0.5 * line.max()]))))
            # the moment maps of every source inside its own box in one pass, and at the peak pixel of
            # source 1 the same two numbers by the three passes of labels.mask(source=1): they are equal
            from katsdpimager_amd import source_maps
            mapper = source_maps.SourceMapsTemplate(ctx, source_maps.SourceMapParameters(
                (0, 1), rest_frequency=rest_frequency)).instantiate(cube_queue, sc.shape)
            own_maps = mapper(labels, sc, catalogue)
            row = catalogue[0]
            box = own_maps.map(1, cube_queue)
            at = (int(row['peak_y'] - row['y0']), int(row['peak_x'] - row['x0']))
            ranged = cube.MomentsTemplate(ctx, cube.MomentParameters(
                (0, 1), rest_frequency=rest_frequency, channels=(int(row['c0']), int(row['c1']) + 1))).instantiate(
                    cube_queue, sc.shape)
            three = ranged(labels.mask(source=1).apply(sc))
            through_mask = tuple(float(three[m].get(cube_queue)[0][row['peak_y'], row['peak_x']]) for m in (0, 1))
            from_map = tuple(float(box[m][at]) for m in (0, 1))
            results['find_sources'].update(first_source_map_shape=box[0].shape, first_source_map=from_map,
                                           first_source_through_mask=through_mask,
                                           source_map_entries=own_maps.total)
            print('source 1 at its peak pixel, from its own {} x {} map (one pass for all {} sources, {} '
                  'entries): moment 0 {:.6f}, moment 1 {:.6f} km/s; through labels.mask(source=1) over its '
                  'channels (three passes): {:.6f}, {:.6f} km/s'.format(
                      box[0].shape[0], box[0].shape[1], len(catalogue), own_maps.total, *from_map,
                      *through_mask))
    if args.output:
        from katsdpimager_amd import io, polarization
        image_p.fixed.polarizations = [polarization.STOKES_I]
        io.write_fits_cube(sc.get(), image_p, args.output, frequencies, (0.0, math.radians(-45.0)),
                           rest_frequency=rest_frequency)
        print('wrote', args.output)
    return results


def _frequencies(obs, channels):
    return 299792458.0 / obs.wavelength + 1.0e5 * np.arange(channels)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--pixels', type=int, default=2048)
    ap.add_argument('--vis', type=int, default=4_000_000)
    ap.add_argument('--major', type=int, default=3)
    ap.add_argument('--minor', type=int, default=500)
    ap.add_argument('--vis-block', type=int, default=1 << 20)
    ap.add_argument('--w-planes', type=int, default=32,
                    help='W planes per slice (more than 64: the kernel table is read from HBM)')
    ap.add_argument('--kernel-width', type=int, default=28)
    ap.add_argument('--output', help='write the restored image to this FITS file')
    ap.add_argument('--mask-radius', type=int, default=0,
                    help='CLEAN only within this many pixels of a source (a mask of disks); 0 = no mask')
    ap.add_argument('--auto-mask', metavar='SIGMA[,RADIUS]',
                    help='build the CLEAN mask from the residual in every major cycle: the pixels SIGMA '
                         'noise estimates above it, grown by RADIUS pixels (default 3); cut to the '
                         '--mask-radius mask if both are given')
    ap.add_argument('--multiscale', metavar='FWHM,FWHM,...',
                    help='run the minor cycles through multi-scale CLEAN with these Gaussian scales '
                         '(FWHM in pixels, ascending, the first one 0), e.g. 0,4,9')
    ap.add_argument('--uvcontsub', metavar='ORDER[:first-last,...]',
                    help='instead of the three-source channel: take a polynomial continuum of this order out of '
                         'a synthetic 16-channel band in the uv plane, the listed channels (default 6-9) holding a line')
    ap.add_argument('--phase-shift', metavar='L,M',
                    help='instead of the default field alone: re-phase the raw visibilities to the direction L,M '
                         'pixels from its centre and image a field a quarter as wide around it, e.g. --phase-shift=-120,60')
    ap.add_argument('--uv-taper', metavar='ARCSEC[,ARCSEC,DEG]',
                    help='instead of the one image: image the channel without and with a Gaussian uv taper '
                         'that alone would give a beam of this FWHM (major, minor, position angle), and print '
                         'the fitted beams and normalized noise, e.g. --uv-taper 30,20,30')
    ap.add_argument('--primary-beam', metavar='FWHM_DEG[,CUTOFF]',
                    help='instead of the one image: attenuate the sources by a cosine-taper primary beam of this '
                         'FWHM, image the channel without and with the primary-beam correction (blanking below '
                         'CUTOFF, default 0.1) and print every source\'s flux before and after, e.g. --primary-beam 0.3 (the default field is 1.2 degrees across)')
    ap.add_argument('--uv-range', metavar='MIN,MAX',
                    help='with or without --uv-taper: keep only the cells between these radii (wavelengths)')
    ap.add_argument('--spectral', metavar='hanning[,N]',
                    help='instead of the three-source channel: Hanning-smooth (and average N channels to one) a '
                         'synthetic band with a line in one channel, and print the line\'s dirty peak in every '
                         'output channel')
    ap.add_argument('--statwt', metavar='TIME_BIN[:first-last,...]',
                    help='instead of the three-source channel: a synthetic band of noise whose sigma differs from '
                         'baseline to baseline under equal weights, imaged without and with the weights rescaled '
                         'from the scatter of groups of TIME_BIN rows (the listed channels left out), e.g. --statwt 8')
    ap.add_argument('--rfiflag', metavar='THRESHOLD', nargs='?', const='',
                    help='instead of the three-source channel: a synthetic band of noise with bursts of '
                         'interference, imaged without and with the SumThreshold flagger (its defaults, or this '
                         'threshold), e.g. --rfiflag 8')
    ap.add_argument('--moments', action='store_true',
                    help='instead of the three-source channel: image a synthetic band with two line sources '
                         'into a spectral cube on the device and print moments 0, 1 and 2 at the sources '
                         'next to what was injected; --output writes the cube')
    ap.add_argument('--imcontsub', metavar='ORDER[:first-last,...]',
                    help='with --moments: leave a continuum source on source A, and fit and subtract a '
                         'polynomial of this order per pixel of the cube outside the listed channels '
                         '(default 1-3,5-10) ahead of the moments, e.g. --imcontsub 1')
    ap.add_argument('--median-contsub', action='store_true',
                    help='with --moments: leave the continuum source on source A and print moment 0 there '
                         'with it left in, after --imcontsub 1 and after the per-pixel median across the '
                         'band has been subtracted (spectrum_stats.SpectrumStats), next to the injected value')
    ap.add_argument('--common-beam', action='store_true',
                    help='with --moments: fit every channel\'s beam, restore the planes with theirs, take the '
                         'cube to the common beam and print moment 0 at source A without and with the smoothing')
    ap.add_argument('--find-sources', action='store_true',
                    help='with --moments: build the smooth-and-clip detection mask of the cube '
                         '(detect.SmoothClip) and print the number of detected voxels and moment 0 at the '
                         'first line source unclipped, with clip_sigma=3 and through the mask; then link the mask '
                         'into sources (link.Link) and print the catalogue and moment 0 of the first source')
    ap.add_argument('--measure-noise', action='store_true',
                    help='with --moments --common-beam: measure the noise of the smoothed planes '
                         '(cube_stats.CubeStats), print it next to the scaled stand-in and use it for the '
                         'clip_sigma moments')
    args = ap.parse_args(argv)
    if args.measure_noise and not args.common_beam:
        ap.error('--measure-noise goes with --moments --common-beam')
    if args.imcontsub and not args.moments:
        ap.error('--imcontsub goes with --moments')
    if args.find_sources and not args.moments:
        ap.error('--find-sources goes with --moments')
    if args.median_contsub and (not args.moments or args.imcontsub or args.common_beam):
        ap.error('--median-contsub goes with --moments, without --imcontsub (it runs both itself) '
                 'and without --common-beam')
    if args.common_beam and not args.moments:
        ap.error('--common-beam goes with --moments')
    if args.moments:
        return moments_band(args)
    if args.rfiflag is not None:
        return rfiflag_band(args)
    if args.statwt:
        return statwt_band(args)
    if args.spectral:
        return spectral_line(args)
    if args.primary_beam:
        return primary_beam_channel(args)
    if args.uv_taper or args.uv_range:
        return uv_taper_channel(args)
    if args.uvcontsub:
        return uvcontsub_band(args)
    if args.phase_shift:
        return phase_shift_field(args)
    import torch
    import scipy.optimize       # noqa: F401  (used by beam.fit_beam; imported here, outside the timings)
    import synth
    from katsdpimager_amd import accel, beam, frontend, imaging, mask, multiscale, parameters, preprocess, weight
    scales = None
    if args.multiscale:
        scales = multiscale.MultiScaleParameters([float(s) for s in args.multiscale.split(',')])
    auto_mask = None
    if args.auto_mask:
        sigma, _, radius = args.auto_mask.partition(',')
        auto_mask = mask.AutoMaskParameters(float(sigma), int(radius) if radius else 3)

    ctx = accel.create_some_context()
    queue = ctx.create_command_queue()
    # array geometry, uvw tracks (metres) and the matching imaging parameters
    obs = synth.make_observation(args.pixels, args.vis, args.w_planes, 1, device=ctx.device)
    image_p, grid_p, array_p = synth.make_parameters(obs, 1, args.kernel_width, degrid=True)
    # three point sources -> raw visibilities (the loader's job in the reference)
    sources = [((40, -25), 1.0), ((-120, 60), 0.5), ((15, 200), 0.25)]      # (l, m) in pixels, Jy
    uvw_wl = obs.uvw.to(torch.float64) / obs.wavelength
    vis = torch.zeros(obs.n_vis, dtype=torch.complex128, device=ctx.device)
    for (lp, mp), flux in sources:
        l, m = lp * obs.pixel_size, mp * obs.pixel_size
        n = math.sqrt(1 - l * l - m * m)
        phase = uvw_wl[:, 0] * l + uvw_wl[:, 1] * m + uvw_wl[:, 2] * (n - 1)
        vis += flux / n * torch.exp(-2j * math.pi * phase)
    vis = vis.to(torch.complex64)[None, :, None].contiguous()
    weights = torch.ones((1, obs.n_vis, 1), dtype=torch.float32, device=ctx.device)

    torch.cuda.synchronize()        # the inputs above were produced on torch's own stream
    t0 = time.perf_counter()
    collector = preprocess.VisibilityCollectorDevice(queue, [image_p], [grid_p], args.vis_block)
    collector.add(accel.DeviceArray(ctx, (obs.n_vis, 3), np.float32, tensor=obs.uvw),
                  accel.DeviceArray(ctx, weights.shape, np.float32, tensor=weights),
                  accel.DeviceArray(ctx, vis.shape, np.complex64, tensor=vis),
                  None, None, np.ones((1, 1), np.complex64), None)
    collector.close()
    reader = collector.reader()
    queue.finish()
    t1 = time.perf_counter()
    print('preprocessed {} visibilities to {} in {:.1f} ms ({:.1f} MB resident)'.format(
        collector.num_input, collector.num_output, (t1 - t0) * 1e3, collector.nbytes() / 1e6))

    weight_p = parameters.WeightParameters(weight.WeightType.ROBUST, 0.0)
    clean_p = parameters.CleanParameters(args.minor, 0.1, 0.85, 5.0, 0, 0.01, 0.5, 0.02)
    template = imaging.ImagingTemplate(ctx, array_p, image_p.fixed, weight_p, grid_p.fixed, clean_p)
    imager = template.instantiate(queue, image_p, grid_p, args.vis_block, 0, args.major, streams=2)
    imager.ensure_all_bound()
    clean_mask = None
    if args.mask_radius > 0:
        yy, xx = np.mgrid[:args.pixels, :args.pixels]
        clean_mask = np.zeros((args.pixels, args.pixels), bool)
        for (lp, mp), _ in sources:
            clean_mask |= ((yy - (args.pixels // 2 + mp)) ** 2 + (xx - (args.pixels // 2 + lp)) ** 2
                           <= args.mask_radius ** 2)
    stats = frontend.process_channel(reader, 0, imager, image_p, grid_p, clean_p,
                                     weight_p.weight_type, args.vis_block, args.major, True,
                                     fit_beam=True, clean_mask=clean_mask, auto_mask=auto_mask,
                                     multiscale=scales)
    queue.finish()
    t2 = time.perf_counter()
    print('imaged in {:.1f} ms: {} major / {} minor cycles, PSF patch {}, noise {:.3g}'.format(
        (t2 - t1) * 1e3, stats['major'], stats['minor'], stats['psf_patch'], stats['noise']))
    if auto_mask is not None:
        print('auto mask ({}): allowed pixels per major cycle {}'.format(auto_mask, stats['mask_pixels']))

    print('restoring beam: {}'.format(stats['restoring_beam']))
    beam.restore(imager, stats['restoring_beam'])
    restored = imager.get_buffer('dirty')[0]
    G = args.pixels
    for (lp, mp), flux in sources:
        y, x = G // 2 + mp, G // 2 + lp
        box = restored[y - 3:y + 4, x - 3:x + 4]
        print('source at (l, m) = ({:5d}, {:5d}) px, {:.2f} Jy: restored peak {:.3f}'.format(
            lp, mp, flux, float(box.max())))
    if args.output:
        from katsdpimager_amd import io, polarization
        image_p.fixed.polarizations = [polarization.STOKES_I]
        io.write_fits_image(imager.get_buffer('dirty'), image_p, args.output, 0,
                            (0.0, math.radians(-45.0)), beam=stats['restoring_beam'])
        print('wrote', args.output)
    return restored, stats


if __name__ == '__main__':
    main()
