"""Smooth-and-clip source mask for a spectral cube: a per-voxel ``clip_sigma`` in :mod:`.cube` collects
positive noise peaks everywhere and misses the faint extended emission that lies below the cut in every
single voxel -- which is what spectral-line work produces.  The field masks by smooth-and-clip instead
(SoFiA's S+C finder, the masks built by hand around CASA ``immoments``, ``tclean``'s auto-multithresh on
cubes): the cube is smoothed with a set of spatial and spectral kernels, each smoothed copy is
thresholded at a multiple of its own measured noise, and the union is the detection mask.

:class:`SmoothClipTemplate` / :class:`SmoothClip` is the finder on the device: csrc/cube_detect.hip's
``kimg_cube_boxcar``, ``kimg_cube_reblank``, ``kimg_cube_threshold`` and ``kimg_cube_mask_prune``
around :mod:`.smooth`'s ``kimg_cube_smooth`` and :mod:`.cube_stats`' ``kimg_cube_stats``, all on one
queue without a host synchronisation.  It returns a :class:`MaskCube`, whose :meth:`MaskCube.apply`
(``kimg_cube_mask_apply``) makes the cube that :class:`cube.Moments` takes unchanged: NaN outside the
mask, which is "not usable" in its contract already.  :func:`boxcar_host`, :func:`reblank_host`,
:func:`threshold_host`, :func:`prune_host` and :func:`apply_host` are the five contracts as numpy and
:func:`smooth_clip_host` the whole finder out of them: the executable specification the device matches
bit for bit.

The contracts (include/kimg.h, "Detection mask").  Cubes are float32 [C][...plane], the mask uint8 of
the same shape (0 = not detected, 1 = detected; any nonzero value reads as set), ``filled`` [C].

* ``boxcar`` (width ``w = 2 h + 1``, odd, 1 to 31): per element, ``z[c']`` is the cube's value where c'
  is in the band, filled, the value finite and the mask (if any) 0 there, else +0.  For every filled c,
  in float64 with c' ascending from ``c - h`` to ``c + h``: ``acc = 0; acc = acc + z[c']``, and
  ``out = float32(acc / w)`` -- always divided by w, which is zero padding.  With ``blank``, NaN where
  the cube itself is not finite.  A direct sum: a running window does not have its bits.
* ``reblank``: NaN into the work cube where the cube is not finite, for filled channels.
* ``threshold``: ``cut = float32(threshold) * sigma[c][g]`` as one float32 product, g = 0 (pooled) or
  the polarization; a finite ``s`` is detected iff ``s > cut`` ('positive'), ``-s > cut`` ('negative')
  or ``|s| > cut`` ('both'); a NaN cut detects nothing.  Detections are OR-ed into the mask.
* ``prune``: per element every run of consecutive set channels shorter than ``min_channels`` is
  cleared, and what stays becomes 1.
* ``apply``: the cube where the mask is set (or, with ``invert``, where it is not), NaN elsewhere, for
  filled channels.

The finder's order is part of the contract: the mask starts at 0; for every spatial FWHM in the order
given and within it every spectral width in the order given, (1) ``boxcar`` into work cube A, reading
the mask as all earlier combinations left it when ``replace`` is set, ``blank`` set iff the FWHM is 0;
(2) for an FWHM above 0, ``kimg_cube_smooth`` from A into B with :func:`gaussian_taps` for every filled
channel, then ``reblank`` of B; (3) ``kimg_cube_stats`` of the result with the parameters' estimator,
border, pooling and the region; (4) ``threshold`` into the mask.  Then ``prune`` if ``min_channels >
1``.  ``region`` and ``border`` limit where the noise is MEASURED, not where voxels may be detected.

Why this order and these rules is DESIGN.md 5.30.

Not done (linking the mask into sources and a catalogue is :mod:`.link`'s): reliability from negative
detections; mask dilation; a running-window boxcar; the noise of a smoothed cube derived rather than measured;
spatial kernels beyond radius 16; ``kimg_moments`` reading the mask itself; cubes across several GPUs.
"""
import ctypes
import math

import numpy as np

from . import accel
from ._lib import lib, check
from .channel_block import integer
from .cube_operator import (MAX_CHANNELS, CubeOperator, CubeTemplate, ReadyArray, SpectralCube, band_size,
                            blank_stale_planes, carry_over, channel_pitch, check_out_cube, host_cube,
                            host_filled, host_plane_mask, is_bool, wait_ready)
from .cube_stats import CubeStatsParameters, cube_stats_host, enqueue_cube_stats, stats_buffers
from .smooth import MAX_RADIUS, _truncate, cube_smooth_host

#: KIMG_BOXCAR_MAX_WIDTH
MAX_WIDTH = 31
#: KIMG_DETECT_POSITIVE, KIMG_DETECT_NEGATIVE, KIMG_DETECT_BOTH
POLARITIES = {'positive': 0, 'negative': 1, 'both': 2}

_QUIET = np.array([0x7fc00000], np.uint32).view(np.float32)[0]


def _width(width):
    if is_bool(width):
        raise ValueError('a width must be an integer, not a bool')
    width = integer(width, 'a spectral width', 1, MAX_WIDTH)
    if width % 2 == 0:
        raise ValueError('a spectral width must be odd')
    return width


def boxcar_host(cube, filled, width, mask=None, blank=False, out=None):
    """The contract of ``kimg_cube_boxcar`` in numpy.  Returns a new array whose unfilled channels are
    ``out``'s (NaN without one)."""
    cube = host_cube(cube, band=True)
    C = cube.shape[0]
    filled = host_filled(filled, C)
    width = _width(width)
    h = width // 2
    usable = np.isfinite(cube) & filled.reshape((C,) + (1,) * (cube.ndim - 1))
    if mask is not None:
        usable &= ~host_plane_mask(mask, cube.shape, 'mask')
    z = np.where(usable, cube, np.float32(0)).astype(np.float64)
    result = np.full(cube.shape, np.nan, np.float32) if out is None else np.array(out, np.float32)
    if result.shape != cube.shape:
        raise ValueError('out has another shape')
    zero = np.zeros(cube.shape[1:], np.float64)
    for c in np.flatnonzero(filled):
        acc = np.zeros(cube.shape[1:], np.float64)
        for k in range(c - h, c + h + 1):
            acc = acc + (z[k] if 0 <= k < C else zero)
        value = (acc / np.float64(width)).astype(np.float32)
        if blank:
            value = np.where(np.isfinite(cube[c]), value, _QUIET)
        result[c] = value
    return result


def reblank_host(work, cube, filled):
    """The contract of ``kimg_cube_reblank`` in numpy: a copy of ``work`` with NaN where a filled
    channel of ``cube`` is not finite."""
    cube = host_cube(cube, band=True)
    work = host_cube(work, 'work', band=True)
    if work.shape != cube.shape:
        raise ValueError('work has another shape')
    filled = host_filled(filled, cube.shape[0])
    result = work.copy()
    for c in np.flatnonzero(filled):
        result[c] = np.where(np.isfinite(cube[c]), work[c], _QUIET)
    return result


def _threshold(value):
    try:
        value = float(value)
    except (TypeError, ValueError):
        raise ValueError('threshold must be a number') from None
    with np.errstate(over='ignore'):
        as_float = np.float32(value)
    if not 0.0 < as_float < np.inf:                 # (false for NaN)
        raise ValueError('threshold must be a finite float32 above 0')
    return as_float


def threshold_host(work, mask, filled, sigma, threshold, polarity='positive'):
    """The contract of ``kimg_cube_threshold`` in numpy.  ``work`` float32 [C][P][H][W]; ``sigma``
    float32 [C][G], G = 1 or P.  Returns a new mask: ``mask`` with the detections set to 1."""
    work = host_cube(work, 'work', band=True)
    if work.ndim != 4:
        raise ValueError('work must be [channel][polarization][y][x]')
    C, P = work.shape[:2]
    filled = host_filled(filled, C)
    mask = np.asarray(mask)
    if mask.dtype != np.uint8 or mask.shape != work.shape:
        raise ValueError('mask must be uint8 of the shape of work')
    sigma = np.asarray(sigma)
    if sigma.dtype != np.float32 or sigma.ndim != 2 or sigma.shape[0] != C or sigma.shape[1] not in (1, P):
        raise ValueError('sigma must be float32 [C][1] or [C][P]')
    threshold = _threshold(threshold)
    if polarity not in POLARITIES:
        raise ValueError("polarity must be 'positive', 'negative' or 'both'")
    result = mask.copy()
    with np.errstate(all='ignore'):
        for c in np.flatnonzero(filled):
            cut = (threshold * sigma[c]).astype(np.float32)
            cut = np.broadcast_to(cut, (P,)).reshape(P, 1, 1)
            s = work[c]
            if polarity == 'positive':
                over = s > cut
            elif polarity == 'negative':
                over = -s > cut
            else:
                over = np.abs(s) > cut
            result[c][np.isfinite(s) & over] = 1
    return result


def prune_host(mask, min_channels):
    """The contract of ``kimg_cube_mask_prune`` in numpy.  Returns a new mask."""
    mask = np.asarray(mask)
    if mask.dtype != np.uint8 or mask.ndim < 2:
        raise ValueError('mask must be uint8 [channel][...plane]')
    C = mask.shape[0]
    if is_bool(min_channels):
        raise ValueError('min_channels must be an integer, not a bool')
    min_channels = integer(min_channels, 'min_channels', 1, C)
    on = mask != 0
    # run[c]: the length of the run of set channels that c belongs to
    before = np.zeros(mask.shape, np.int64)
    after = np.zeros(mask.shape, np.int64)
    for c in range(C):
        before[c] = np.where(on[c], (before[c - 1] if c else 0) + 1, 0)
    for c in range(C - 1, -1, -1):
        after[c] = np.where(on[c], (after[c + 1] if c + 1 < C else 0) + 1, 0)
    run = before + after - 1
    return (on & (run >= min_channels)).astype(np.uint8)


def apply_host(cube, mask, filled, invert=False, out=None):
    """The contract of ``kimg_cube_mask_apply`` in numpy.  Returns a new array whose unfilled channels
    are ``out``'s (the cube's own without one, as in place)."""
    cube = host_cube(cube, band=True)
    filled = host_filled(filled, cube.shape[0])
    keep = host_plane_mask(mask, cube.shape, 'mask') != bool(invert)
    result = cube.copy() if out is None else np.array(out, np.float32)
    if result.shape != cube.shape:
        raise ValueError('out has another shape')
    for c in np.flatnonzero(filled):
        result[c] = np.where(keep[c], cube[c], _QUIET)
    return result


def gaussian_taps(fwhm, truncate=3.0):
    """``(radius, float32 taps [(2 radius + 1)^2])`` of a round Gaussian of ``fwhm`` pixels for
    ``kimg_cube_smooth``: ``sigma = fwhm / (2 sqrt(2 ln 2))``, ``radius = ceil(truncate * sigma)``, the
    taps sampled at pixel centres in float64, row-major, divided by their sum (float64, summed one by
    one in that order) and rounded once.  ``fwhm == 0`` gives radius 0 and the single tap 1.
    ValueError for a radius above ``smooth.MAX_RADIUS``."""
    try:
        fwhm = float(fwhm)
    except (TypeError, ValueError):
        raise ValueError('a spatial FWHM must be a number') from None
    if not 0.0 <= fwhm < np.inf:                    # (false for NaN)
        raise ValueError('a spatial FWHM must be finite and not below 0')
    truncate = _truncate(truncate)
    if fwhm == 0.0:
        return 0, np.ones(1, np.float32)
    sigma = fwhm / (2.0 * math.sqrt(2.0 * math.log(2.0)))
    radius = int(math.ceil(truncate * sigma))
    if radius > MAX_RADIUS:
        raise ValueError('an FWHM of {} px needs a kernel of radius {} > {}'.format(fwhm, radius, MAX_RADIUS))
    d = np.arange(-radius, radius + 1, dtype=np.float64)
    g = np.exp(-0.5 * (d[:, np.newaxis] ** 2 + d[np.newaxis, :] ** 2) / (sigma * sigma)).reshape(-1)
    total = 0.0
    for x in g:                 # (row-major, one by one: the order is part of the contract)
        total += x
    return radius, (g / total).astype(np.float32)


class SmoothClipParameters:
    """``spatial_fwhm``: the FWHMs (pixels, 0 = none) of the round Gaussians, in the order they are
    run; ``spectral_widths``: the boxcar widths (channels, odd, 1 to 31), in the order they are run
    within every FWHM.  ``threshold``: a voxel of a smoothed copy is detected above this many of the
    copy's own measured sigma.  ``polarity``: 'positive', 'negative' or 'both'.  ``estimator``,
    ``pool_polarizations``, ``border``: how the sigma of every plane is measured
    (:class:`cube_stats.CubeStatsParameters`); ``border`` and the ``region`` of a call limit where the
    noise is measured, not where voxels may be detected.  ``replace``: voxels that an earlier
    combination detected enter the later ones as 0 (SoFiA's replacement, which keeps a bright source
    from being smeared into a halo of detections).  ``min_channels``: runs of detected channels shorter
    than this are dropped at the end.  ``truncate``: a spatial kernel reaches out to this many of its
    sigma."""

    def __init__(self, spatial_fwhm=(0, 3, 6), spectral_widths=(1, 3, 7), threshold=5.0,
                 polarity='positive', estimator='median_abs', pool_polarizations=True, border=0,
                 replace=True, min_channels=1, truncate=3.0):
        self.truncate = _truncate(truncate)
        if isinstance(spatial_fwhm, str) or isinstance(spectral_widths, str):
            raise ValueError('spatial_fwhm and spectral_widths must be sequences of numbers')
        try:
            spatial_fwhm = tuple(spatial_fwhm)
            spectral_widths = tuple(spectral_widths)
        except TypeError:
            raise ValueError('spatial_fwhm and spectral_widths must be sequences') from None
        if not spatial_fwhm or not spectral_widths:
            raise ValueError('no smoothing kernel asked for')
        for fwhm in spatial_fwhm:
            if is_bool(fwhm):
                raise ValueError('a spatial FWHM must be a number, not a bool')
            gaussian_taps(fwhm, self.truncate)
        self.spatial_fwhm = tuple(float(fwhm) for fwhm in spatial_fwhm)
        self.spectral_widths = tuple(_width(width) for width in spectral_widths)
        self.threshold = float(_threshold(threshold))
        if not isinstance(polarity, str) or polarity not in POLARITIES:
            raise ValueError("polarity must be 'positive', 'negative' or 'both'")
        self.polarity = polarity
        # (estimator, border and pool_polarizations are validated as cube_stats' own)
        self.stats = CubeStatsParameters(estimator=estimator, border=border,
                                         pool_polarizations=pool_polarizations)
        self.estimator = self.stats.estimator
        self.border = self.stats.border
        self.pool_polarizations = self.stats.pool_polarizations
        if not is_bool(replace):
            raise ValueError('replace must be a bool')
        self.replace = bool(replace)
        if is_bool(min_channels):
            raise ValueError('min_channels must be an integer, not a bool')
        self.min_channels = integer(min_channels, 'min_channels', 1, MAX_CHANNELS)

    def check_shape(self, shape):
        """ValueError unless cubes of ``shape`` = (C, P, H, W) can be searched."""
        C, P, H, W = shape
        band_size(C)
        if self.min_channels > C:
            raise ValueError('min_channels {} in a cube of {} channels'.format(self.min_channels, C))
        self.stats.check_plane(H, W)
        if (P if self.pool_polarizations else 1) * H * W >= 2 ** 32:
            raise ValueError('a group of 2^32 elements or more')

    def __repr__(self):
        return ('SmoothClipParameters(spatial_fwhm={!r}, spectral_widths={!r}, threshold={!r}, '
                'polarity={!r}, estimator={!r}, pool_polarizations={!r}, border={!r}, replace={!r}, '
                'min_channels={!r}, truncate={!r})').format(
                    self.spatial_fwhm, self.spectral_widths, self.threshold, self.polarity,
                    self.estimator, self.pool_polarizations, self.border, self.replace,
                    self.min_channels, self.truncate)


def smooth_clip_host(cube, filled, params, region=None):
    """The whole finder in numpy, out of the twins above, ``smooth.cube_smooth_host`` and
    ``cube_stats.cube_stats_host``, in the order of the module's docstring.  ``cube`` float32
    [C][P][H][W]; ``filled`` [C]; ``region`` None or uint8/bool [H][W]: where the noise is measured
    (not where voxels may be detected).  Returns the mask, uint8 [C][P][H][W]."""
    if not isinstance(params, SmoothClipParameters):
        raise TypeError('params must be SmoothClipParameters')
    cube = host_cube(cube, band=True)
    if cube.ndim != 4:
        raise ValueError('cube must be [channel][polarization][y][x]')
    C = cube.shape[0]
    filled = host_filled(filled, C)
    params.check_shape(cube.shape)
    mask = np.zeros(cube.shape, np.uint8)
    for fwhm in params.spatial_fwhm:
        radius, taps = gaussian_taps(fwhm, params.truncate)
        for width in params.spectral_widths:
            work = boxcar_host(cube, filled, width, mask if params.replace else None, blank=fwhm == 0)
            if fwhm > 0:
                work = cube_smooth_host(work, filled, np.full(C, radius, np.int32),
                                        np.tile(taps, (C, 1)))
                work = reblank_host(work, cube, filled)
            sigma = cube_stats_host(work, filled, params.stats, region).sigma
            mask = threshold_host(work, mask, filled, sigma, params.threshold, params.polarity)
    if params.min_channels > 1:
        mask = prune_host(mask, params.min_channels)
    return mask


class MaskCube(ReadyArray):
    """A detection mask, device uint8 [C][P][H][W]: 0 = not detected, 1 = detected; a
    :class:`cube_operator.ReadyArray`, whose ``filled`` (uint8 [C]) is what the finder was told."""

    def apply(self, cube, out=None, invert=False):
        """``kimg_cube_mask_apply``: the :class:`cube.SpectralCube` ``cube`` with NaN where the mask is
        not set (``invert``: where it is set), in every filled channel, on the mask's queue.  ``out``
        None: a new SpectralCube, which carries ``filled``, ``noise``, ``beams``, the common beam and
        the frequencies over; ``out`` the cube itself: in place; another SpectralCube of the same
        shape and frequencies: into it, likewise.  Returns the cube written, which
        :class:`cube.Moments` takes as it is: NaN is "not usable" there."""
        if not isinstance(cube, SpectralCube):
            raise TypeError('cube must be a SpectralCube')
        if tuple(cube.shape) != self.shape:
            raise ValueError('a mask of {} for a cube of {}'.format(self.shape, tuple(cube.shape)))
        if not is_bool(invert):
            raise ValueError('invert must be a bool')
        check_out_cube(cube, out, 'masked cube', same=('shape', 'frequencies'))
        queue = self.command_queue
        if out is None:
            out = SpectralCube.like(cube, queue)
        filled = np.ascontiguousarray(cube.filled != 0, np.uint8)
        wait_ready(queue, self)
        cube.array.used_on(queue)
        out.array.used_on(queue)
        self.used_on(queue)
        C = self.shape[0]
        M = int(np.prod(self.shape[1:]))
        out_pitch = channel_pitch(out.array)
        if out is not cube:
            blank_stale_planes(queue, out.array, out_pitch,
                               np.flatnonzero((out.filled != 0) & (filled == 0)), M)
        check(lib().kimg_cube_mask_apply(
            cube.array.ptr, channel_pitch(cube.array), self.ptr, M, out.array.ptr, out_pitch, C, M,
            filled.ctypes.data_as(ctypes.c_void_p), int(invert), queue.handle), 'kimg_cube_mask_apply')
        carry_over(cube, out, beams=True)
        return out


class SmoothClip(CubeOperator):
    """The smooth-and-clip finder for cubes of shape ``cube_shape`` = (C, P, H, W).  ``op(the_cube,
    region=None)`` takes a :class:`cube.SpectralCube` and returns a :class:`MaskCube`;
    ``op(array, filled=..., region=None)`` takes a plain :class:`accel.DeviceArray` [C][P][H][W] whose
    [P][H][W] plane is dense while the channel axis may have any pitch.  ``region``: a device array
    (``primary_beam``'s ``beam_valid`` will do) or a host array, which is uploaded before the first
    launch; uint8 or bool [H][W].  It and ``border`` limit where the noise is measured, not where
    voxels may be detected.

    The operator owns two work cubes, the statistics' scratch and tables and the spatial taps, all
    allocated at ``instantiate``; a call allocates the mask, is a fixed sequence of launches on
    ``command_queue`` and never waits for the device.  The cube is never written."""

    def __init__(self, template, command_queue, cube_shape):
        super().__init__(template, command_queue, cube_shape)
        params = self.params
        queue = command_queue
        params.check_shape(self.cube_shape)
        C, P, H, W = self.cube_shape
        context = queue.context
        self.groups = params.stats.groups(P)
        self._work = [accel.DeviceArray(context, self.cube_shape, np.float32, queue=queue)
                      for _ in range(2 if any(f > 0 for f in params.spatial_fwhm) else 1)]
        self._scratch, self._stats = stats_buffers(queue, C, self.groups)
        # per FWHM above 0: (radius int32 [C], taps on the device [C][(2 R + 1)^2], the same row for
        # every channel: kimg_cube_smooth has a kernel per channel)
        self._taps = {}
        for fwhm in params.spatial_fwhm:
            if fwhm > 0 and fwhm not in self._taps:
                radius, taps = gaussian_taps(fwhm, params.truncate)
                table = accel.DeviceArray(context, (C, taps.size), np.float32, queue=queue)
                table.set(queue, np.tile(taps, (C, 1)))
                self._taps[fwhm] = (np.full(C, radius, np.int32), table)

    def __call__(self, cube, filled=None, region=None):
        params = self.params
        C, P, H, W = self.cube_shape
        M = P * H * W
        queue = self.command_queue
        array = self._array(cube, 'cube')
        filled = self._filled(self._own_filled(cube, filled))
        pitch = channel_pitch(array)
        region_ptr = None if region is None else self._device_region(region).ptr
        mask = MaskCube.of_cube(queue, self.cube_shape, np.uint8, filled)
        mask.zero(queue)
        array.used_on(queue)
        handle = queue.handle
        filled_ptr = filled.ctypes.data_as(ctypes.c_void_p)
        sigma_ptr = self._stats.ptr + 4 * 4 * C * self.groups      # (the fifth table)
        A = self._work[0]
        for fwhm in params.spatial_fwhm:
            for width in params.spectral_widths:
                check(lib().kimg_cube_boxcar(
                    array.ptr, pitch, mask.ptr if params.replace else None, M, A.ptr, M, C, M,
                    filled_ptr, width, int(fwhm == 0), handle), 'kimg_cube_boxcar')
                work = A
                if fwhm > 0:
                    work = self._work[1]
                    radius, taps = self._taps[fwhm]
                    check(lib().kimg_cube_smooth(
                        A.ptr, M, work.ptr, M, C, P, H, W, filled_ptr,
                        radius.ctypes.data_as(ctypes.c_void_p), taps.ptr, taps.shape[1], handle),
                        'kimg_cube_smooth')
                    check(lib().kimg_cube_reblank(work.ptr, M, array.ptr, pitch, C, M, filled_ptr,
                                                  handle), 'kimg_cube_reblank')
                enqueue_cube_stats(queue, work.ptr, M, self.cube_shape, filled, 0, C, params.stats,
                                   region_ptr, self._scratch, self._stats)
                check(lib().kimg_cube_threshold(
                    work.ptr, M, mask.ptr, M, C, P, H, W, filled_ptr, sigma_ptr, self.groups,
                    params.threshold, POLARITIES[params.polarity], handle), 'kimg_cube_threshold')
        if params.min_channels > 1:
            check(lib().kimg_cube_mask_prune(mask.ptr, M, C, M, params.min_channels, handle),
                  'kimg_cube_mask_prune')
        mask.ready = queue.enqueue_marker()
        return mask


class SmoothClipTemplate(CubeTemplate):
    params_type = SmoothClipParameters
    operator = SmoothClip
