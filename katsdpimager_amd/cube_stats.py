"""Cube plane statistics: for every plane of a spectral cube a robust noise and its companion
statistics -- count, min, max, median -- in one call on the device (CASA ``imstat`` per channel,
MIRIAD ``imstat`` / ``sigest``).  It measures what :class:`cube.MomentParameters` (``clip_sigma``)
and :class:`imcontsub.ImContSubParameters` (``weighting='noise'``) read, on a cube whose planes did
not come with a noise from ``frontend.process_channel``: one that :mod:`.smooth` took to a common
beam (its smoothed planes have ``noise = NaN``), one that :mod:`.imcontsub` wrote, one filled from
the host or from other GPUs.  The chain then closes: image, ``put(beam=)``, common beam, measure,
``imcontsub(weighting='noise')``, moments with ``clip_sigma``.

:class:`CubeStatsTemplate` / :class:`CubeStats` is the operator (csrc/cube_stats.hip,
``kimg_cube_stats``); :func:`cube_stats_host` is the same contract as numpy and the executable
specification the device matches bit for bit.

The contract (include/kimg.h, "Cube plane statistics").

* Input: ``cube`` float32 [C][P][H][W], the [P][H][W] plane dense, the channel axis of any pitch of
  at least ``P * H * W``; ``filled`` host uint8 [C]; ``channels = (first, stop)``.  The cube is never
  written.
* Groups: ``G = 1`` a channel with ``pool_polarizations`` (the default; what ``process_channel``'s
  noise is: one number a channel over all P), else ``G = P``.  A group's candidates are the pixels of
  its plane(s) with ``border <= y < H - border`` and ``border <= x < W - border`` (``border`` in
  pixels, 0 or more, ``2 * border < min(H, W)``) and ``region[y][x] != 0`` where a ``region`` (uint8
  or bool [H][W], shared by all channels and polarizations) is given.
* Samples: a candidate is a sample iff its value is finite: NaN of any sign or payload, +Inf and -Inf
  are left out.  ``count`` (uint32) is the number of samples n.  Groups of 2^32 elements or more are
  refused.
* Order: by integer key, the monotone map of the float32 bit pattern (:func:`keys`): -0 lies below
  +0.  Nothing depends on launch geometry.
* Median of a multiset v of n >= 1 float32 values: ``lo = v[(n - 1) // 2]``, ``hi = v[n // 2]``,
  ``(lo + hi) / 2`` in float32 (``kimg_noise_est``'s rule, ``np.median`` of float32 data).
* Outputs per group: ``min``, ``max``, ``median`` of the samples, and ``sigma``:
  ``estimator='median_abs'`` (the default, the imager's own) ``median(|x|) *
  float32(1.4826022185056031)`` as one float32 product, ``|x|`` the value with its sign bit cleared;
  ``estimator='mad'`` ``median(|x - m|)`` times the same constant, m the group's median, ``x - m`` one
  float32 subtraction with its sign bit cleared.
* A group with n == 0 has NaN in the four float outputs and count 0, and so has every group of a
  channel that is unfilled or outside the range; unfilled channels are not read.
* Everything is exact selection: no sums, nothing rounds but the operations above, so twin and
  device agree bit for bit, always.  On a plane without non-finite values, pooled, without region and
  with the same border in pixels, ``sigma`` under 'median_abs' is :class:`clean.NoiseEst`'s, by bits.

Not done: iterative sigma clipping; means and rms (they need an ordered float64 reduction and are
another contract); the noise of a smoothed plane derived rather than measured; cubes across several
GPUs.  Per-pixel statistics along the channel axis (the "medians" of ``immoments``) are
:mod:`.spectrum_stats`.
"""
import ctypes

import numpy as np

from . import accel
from ._lib import lib, check
from .channel_block import integer
from .cube_operator import (CubeOperator, CubeTemplate, SpectralCube, channel_pitch, channel_range,
                            host_cube, host_filled, host_plane_mask, is_bool, range_in_band)

#: KIMG_CUBE_STATS_MEDIAN_ABS, KIMG_CUBE_STATS_MAD
ESTIMATORS = {'median_abs': 0, 'mad': 1}
#: KIMG_CUBE_STATS_TO_RMS: sigma of a Gaussian over its median absolute deviation
TO_RMS = np.float32(1.4826022185056031)

_FIELDS = ('count', 'min', 'max', 'median', 'sigma')


class CubeStatsParameters:
    """``estimator``: 'median_abs' or 'mad' (the module's docstring).  ``border``: pixels left out
    along every edge of a plane, an integer.  ``pool_polarizations``: one group a channel over all
    polarizations (True), or one a plane.  ``channels`` = (first, stop), default the whole band."""

    def __init__(self, estimator='median_abs', border=0, pool_polarizations=True, channels=None):
        if not isinstance(estimator, str) or estimator not in ESTIMATORS:
            raise ValueError("estimator must be 'median_abs' or 'mad'")
        self.estimator = estimator
        if is_bool(border):
            raise ValueError('border must be an integer, not a bool')
        self.border = integer(border, 'border', 0, 2 ** 30)
        if not is_bool(pool_polarizations):
            raise ValueError('pool_polarizations must be a bool')
        self.pool_polarizations = bool(pool_polarizations)
        self.channels = None if channels is None else channel_range(channels, 'channels')

    def range(self, num_channels):
        """(first, stop) within a band of ``num_channels`` channels."""
        return range_in_band(self.channels, num_channels)

    def groups(self, num_polarizations):
        """G: groups per channel."""
        return 1 if self.pool_polarizations else int(num_polarizations)

    def check_plane(self, height, width):
        if 2 * self.border >= min(height, width):
            raise ValueError('a border of {} leaves nothing of a {} x {} plane'.format(
                self.border, height, width))

    def __repr__(self):
        return 'CubeStatsParameters(estimator={!r}, border={!r}, pool_polarizations={!r}, channels={!r})'.format(
            self.estimator, self.border, self.pool_polarizations, self.channels)


class CubeStatsResult:
    """Host arrays [C][G]: ``count`` (uint32) and ``min``, ``max``, ``median``, ``sigma`` (float32)."""

    def __init__(self, count, min, max, median, sigma):
        self.count = count
        self.min = min
        self.max = max
        self.median = median
        self.sigma = sigma

    def __repr__(self):
        return 'CubeStatsResult({} channels x {} groups)'.format(*self.count.shape)


def keys(values):
    """The integer key of float32 values: ``bits ^ (0xffffffff if bits >> 31 else 0x80000000)``,
    uint32, monotone in the value, -0 below +0."""
    bits = np.ascontiguousarray(values, np.float32).view(np.uint32)
    return bits ^ np.where(bits >> 31 != 0, np.uint32(0xffffffff), np.uint32(0x80000000))


def values_of(key):
    """The float32 values of integer keys (the inverse of :func:`keys`)."""
    key = np.ascontiguousarray(key, np.uint32)
    bits = np.where(key >> 31 != 0, key ^ np.uint32(0x80000000), ~key)
    return bits.astype(np.uint32).view(np.float32)


def _median(ordered):
    """``(lo + hi) / 2`` in float32 of values in key order."""
    n = len(ordered)
    with np.errstate(all='ignore'):
        return np.float32(np.float32(ordered[(n - 1) // 2] + ordered[n // 2]) / np.float32(2))


def _sorted(values):
    return values_of(np.sort(keys(values)))


def cube_stats_host(cube, filled, params, region=None):
    """The contract of ``kimg_cube_stats`` (include/kimg.h) in numpy: per group the finite candidates
    sorted by integer key and indexed.  ``cube`` float32 [C][P][H][W]; ``filled`` [C]; ``region``
    None or uint8/bool [H][W].  Returns a :class:`CubeStatsResult`."""
    if not isinstance(params, CubeStatsParameters):
        raise TypeError('params must be CubeStatsParameters')
    cube = host_cube(cube, ndim=4)
    C, P, H, W = cube.shape
    filled = host_filled(filled, C)
    first, stop = params.range(C)
    params.check_plane(H, W)
    G = params.groups(P)
    if (P if G == 1 else 1) * H * W >= 2 ** 32:
        raise ValueError('a group of 2^32 elements or more')
    b = params.border
    candidate = np.zeros((H, W), bool)
    candidate[b:H - b, b:W - b] = True
    if region is not None:
        candidate &= host_plane_mask(region, (H, W), 'region')
    count = np.zeros((C, G), np.uint32)
    out = {name: np.full((C, G), np.nan, np.float32) for name in _FIELDS[1:]}
    for c in range(first, stop):
        if not filled[c]:
            continue
        for g in range(G):
            planes = cube[c] if G == 1 else cube[c, g:g + 1]
            x = planes[:, candidate]
            x = x[np.isfinite(x)]
            if not x.size:
                continue
            ordered = _sorted(x)
            count[c, g] = x.size
            out['min'][c, g] = ordered[0]
            out['max'][c, g] = ordered[-1]
            m = _median(ordered)
            out['median'][c, g] = m
            with np.errstate(all='ignore'):
                v = x if params.estimator == 'median_abs' else (x - m).astype(np.float32)
            spread = (v.view(np.uint32) & np.uint32(0x7fffffff)).view(np.float32)
            with np.errstate(all='ignore'):
                out['sigma'][c, g] = np.float32(_median(_sorted(spread)) * TO_RMS)
    return CubeStatsResult(count, out['min'], out['max'], out['median'], out['sigma'])


def record_noise(the_cube, result, params):
    """``update_noise``: ``sigma[:, 0]`` into ``the_cube.noise`` for the filled channels of the range;
    the others are left alone.  Pooled results only."""
    if not params.pool_polarizations:
        raise ValueError('update_noise needs pool_polarizations: a cube records one noise a channel')
    first, stop = params.range(the_cube.shape[0])
    for c in range(first, stop):
        if the_cube.filled[c]:
            the_cube.noise[c] = result.sigma[c, 0]


def stats_buffers(queue, num_channels, groups):
    """``(scratch, out)`` of :func:`enqueue_cube_stats` for C channels of G groups: the library's
    scratch and the five tables, uint32 [5][C][G]."""
    words = lib().kimg_cube_stats_scratch_bytes(num_channels, groups) // 4
    return (accel.DeviceArray(queue.context, (words,), np.uint32, queue=queue),
            accel.DeviceArray(queue.context, (5, num_channels, groups), np.uint32, queue=queue))


def enqueue_cube_stats(queue, array_ptr, pitch, shape, filled, first, stop, params, region_ptr,
                       scratch, out):
    """One ``kimg_cube_stats`` on ``queue``: the cube of ``shape`` = (C, P, H, W) at ``array_ptr``
    with the channel ``pitch``, ``filled`` the host uint8 [C], ``params`` the
    :class:`CubeStatsParameters`; ``out[k]`` takes field k of ``_FIELDS``."""
    C, P, H, W = shape
    step = 4 * C * params.groups(P)
    check(lib().kimg_cube_stats(
        array_ptr, pitch, C, P, H, W, filled.ctypes.data_as(ctypes.c_void_p), first, stop,
        int(params.pool_polarizations), ESTIMATORS[params.estimator], params.border, region_ptr,
        scratch.ptr, *(out.ptr + k * step for k in range(5)), queue.handle), 'kimg_cube_stats')


class CubeStats(CubeOperator):
    """``kimg_cube_stats`` for cubes of shape ``cube_shape`` = (C, P, H, W).  ``op(the_cube,
    region=None, update_noise=False)`` takes a :class:`cube.SpectralCube` and returns a
    :class:`CubeStatsResult`; ``update_noise=True`` (pooled only) writes ``sigma[:, 0]`` into
    ``the_cube.noise`` for the filled channels of the range.  ``op(array, filled=..., region=None)``
    takes a plain :class:`accel.DeviceArray` [C][P][H][W] whose [P][H][W] plane is dense while the
    channel axis may have any pitch.  ``region``: a device array (``primary_beam``'s ``beam_valid``
    will do) or a host array, which is uploaded; uint8 or bool [H][W].

    One call is a fixed number of launches whatever C is (9 for 'median_abs', 17 for 'mad') and ends
    with the one read of the ``5 * C * G`` numbers, so it waits for the queue."""

    def __init__(self, template, command_queue, cube_shape):
        super().__init__(template, command_queue, cube_shape, band=True)
        C, P, H, W = self.cube_shape
        self.range = self.params.range(C)
        self.params.check_plane(H, W)
        self.groups = self.params.groups(P)
        if (P if self.groups == 1 else 1) * H * W >= 2 ** 32:
            raise ValueError('a group of 2^32 elements or more')
        self._scratch = self._out = None

    def __call__(self, cube, filled=None, region=None, update_noise=False):
        params = self.params
        queue = self.command_queue
        array = self._array(cube, 'cube')
        if not is_bool(update_noise):
            raise ValueError('update_noise must be a bool')
        filled = self._own_filled(cube, filled)
        if update_noise and not isinstance(cube, SpectralCube):
            raise ValueError('update_noise needs a SpectralCube')
        if update_noise and not params.pool_polarizations:
            raise ValueError('update_noise needs pool_polarizations: a cube records one noise a channel')
        filled = self._filled(filled)
        pitch = channel_pitch(array)
        region_ptr = None if region is None else self._device_region(region).ptr
        if self._scratch is None:
            self._scratch, self._out = stats_buffers(queue, self.cube_shape[0], self.groups)
        array.used_on(queue)
        enqueue_cube_stats(queue, array.ptr, pitch, self.cube_shape, filled, *self.range, params,
                           region_ptr, self._scratch, self._out)
        words = self._out.get(queue)
        result = CubeStatsResult(words[0].copy(), *(words[i].view(np.float32).copy() for i in range(1, 5)))
        if update_noise:
            record_noise(cube, result, params)
        return result


class CubeStatsTemplate(CubeTemplate):
    params_type = CubeStatsParameters
    operator = CubeStats

