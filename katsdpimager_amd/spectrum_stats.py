"""Spectrum statistics: for every pixel of a spectral cube the statistics of its own spectrum --
count, min, max, median and a robust sigma along the channel axis -- as maps [P][H][W], and
optionally the cube with that median subtracted from every filled channel.

Two things a spectral-line user does with them.  The ``sigma`` map is a per-pixel noise: after
:mod:`.primary_beam` correction the noise grows towards the edge of the field and the one number a
channel of :mod:`.cube_stats` is wrong almost everywhere; source finders scale by the MAD of every
pixel's own spectrum.  The ``median`` map is a continuum estimate that needs no line ranges:
:mod:`.imcontsub` must be told where the line is, the median across the band needs nothing as long as
the line fills less than half of it (CASA ``immoments`` moment 3, MIRIAD ``contsub``'s median mode);
``subtract=True`` takes it out of the cube.

:class:`SpectrumStatsTemplate` / :class:`SpectrumStats` is the operator (csrc/spectrum_stats.hip,
``kimg_spectrum_stats``); :func:`spectrum_stats_host` is the same contract as numpy and the
executable specification the device matches bit for bit.

The contract (include/kimg.h, "Spectrum statistics").

* Input: ``cube`` float32 [C][...plane], the plane dense, the channel axis of any pitch; ``filled``
  host uint8 [C].  A channel ENTERS iff it lies in ``channels = (first, stop)``, outside every range of
  ``exclude_ranges`` (a list of ``(first, last + 1)``, the negative of ``imcontsub``'s ``line_ranges``)
  and is filled.  S entering channels; S = 0 gives n = 0 everywhere.
* Per element: the samples are the finite values of the entering channels, n their count.  Order is by
  :func:`cube_stats.keys` (-0 below +0).  ``median = (v[(n - 1) // 2] + v[n // 2]) / 2`` in float32
  (it may overflow to Inf); ``min`` and ``max`` the samples of smallest and largest key; ``sigma``
  under 'mad' ``median(|x - median|) * TO_RMS`` with ``x - median`` one float32 subtraction, under
  'median_abs' ``median(|x|) * TO_RMS``; ``count`` = n (int32), always.
* ``min_samples`` (>= 1): the four float maps are NaN where ``n < min_samples``.
* ``line``: for every FILLED channel of the whole band -- not only the entering ones -- ``cube[c] -
  median`` as one float32 subtraction, NaN where ``n < min_samples``; channels that are not filled are
  neither read nor written.
* Everything is exact selection plus single float32 operations: twin and device agree bit for bit,
  in either kernel form.

Not done: moments 4 to 7, the coordinate of the minimum (moment 11), a per-pixel cut in
:class:`cube.Moments` made from these maps, iterative clipping, robust polynomial fits.
"""
import ctypes

import numpy as np

from ._lib import lib, check
from .channel_block import OperatorTemplate, integer
from .cube_operator import (CubeOperator, MapArray, carry_over, channel_pitch, channel_range,
                            check_out_cube, host_cube, host_filled, is_bool, mark_ready, range_in_band)
from .cube_stats import ESTIMATORS, TO_RMS, keys, values_of

#: KIMG_SPECTRUM_* of include/kimg.h
OUTPUT_BITS = {'median': 1, 'sigma': 2, 'min': 4, 'max': 8, 'count': 16}
DEFAULT_OUTPUTS = ('median', 'sigma', 'count')
#: KIMG_SPECTRUM_FORM_*
FORMS = {'auto': 0, 'resident': 1, 'streaming': 2}

_NONE = np.uint64(1) << np.uint64(32)       # above every key: what is not a sample


class SpectrumStatsParameters:
    """``estimator``: 'mad' (the default here: a spectrum sits on its continuum) or 'median_abs'.
    ``channels`` = (first, stop), default the whole band.  ``exclude_ranges``: a list of
    ``(first, last + 1)`` channel ranges left OUT of the statistics (``imcontsub``'s ``line_ranges``
    will do), default none.  ``min_samples``: the float maps are NaN with fewer finite samples, 1 or
    more.  ``outputs``: distinct names from 'median', 'sigma', 'min', 'max', 'count'."""

    def __init__(self, estimator='mad', channels=None, exclude_ranges=None, min_samples=1,
                 outputs=DEFAULT_OUTPUTS):
        if not isinstance(estimator, str) or estimator not in ESTIMATORS:
            raise ValueError("estimator must be 'median_abs' or 'mad'")
        self.estimator = estimator
        self.channels = None if channels is None else channel_range(channels, 'channels')
        self.exclude_ranges = None
        if exclude_ranges is not None:
            try:
                ranges = list(exclude_ranges)
            except TypeError:
                raise ValueError('exclude_ranges must be a list of (first, stop)') from None
            self.exclude_ranges = [channel_range(r, 'an excluded range') for r in ranges]
        if is_bool(min_samples):
            raise ValueError('min_samples must be an integer, not a bool')
        self.min_samples = integer(min_samples, 'min_samples', 1, 2 ** 31 - 1)
        if isinstance(outputs, str):
            raise ValueError('outputs must be a sequence of map names')
        try:
            outputs = tuple(outputs)
        except TypeError:
            raise ValueError('outputs must be a sequence of map names') from None
        if not outputs or len(set(outputs)) != len(outputs) \
                or any(not isinstance(name, str) or name not in OUTPUT_BITS for name in outputs):
            raise ValueError('outputs must be distinct names from {}'.format(sorted(OUTPUT_BITS)))
        self.outputs = outputs

    def range(self, num_channels):
        """(first, stop) within a band of ``num_channels`` channels."""
        return range_in_band(self.channels, num_channels)

    def stat(self, num_channels):
        """uint8 [C]: 1 where ``exclude_ranges`` lets a channel in (the range and ``filled`` come on
        top of it)."""
        self.range(num_channels)
        stat = np.ones(int(num_channels), np.uint8)
        for first, stop in self.exclude_ranges or ():
            if stop > num_channels:
                raise ValueError('excluded range ({}, {}) beyond the {} channels'.format(
                    first, stop, num_channels))
            stat[first:stop] = 0
        return stat

    def entering(self, num_channels, filled):
        """bool [C]: the channels that enter the statistics."""
        first, stop = self.range(num_channels)
        filled = host_filled(filled, num_channels)
        enter = (self.stat(num_channels) != 0) & filled
        enter[:first] = False
        enter[stop:] = False
        return enter

    def __repr__(self):
        text = 'SpectrumStatsParameters(estimator={!r}'.format(self.estimator)
        if self.channels is not None:
            text += ', channels={!r}'.format(self.channels)
        if self.exclude_ranges is not None:
            text += ', exclude_ranges={!r}'.format(self.exclude_ranges)
        return text + ', min_samples={!r}, outputs={!r})'.format(self.min_samples, self.outputs)


def _middle(ordered, n):
    """``(v[(n - 1) // 2] + v[n // 2]) / 2`` in float32 per column of keys sorted along axis 0 (uint64,
    what is not a sample last); columns with n == 0 give anything."""
    if ordered.shape[0] == 0:
        return np.zeros(ordered.shape[1:], np.float32)
    at = np.maximum(n, 1)
    lo = np.take_along_axis(ordered, ((at - 1) // 2)[np.newaxis], 0)[0]
    hi = np.take_along_axis(ordered, np.minimum(at // 2, ordered.shape[0] - 1)[np.newaxis], 0)[0]
    lo = values_of((lo & np.uint64(0xffffffff)).astype(np.uint32))
    hi = values_of((hi & np.uint64(0xffffffff)).astype(np.uint32))
    with np.errstate(all='ignore'):
        return ((lo + hi).astype(np.float32) / np.float32(2)).astype(np.float32)


def spectrum_stats_host(cube, filled, params, subtract=False):
    """The contract of ``kimg_spectrum_stats`` (include/kimg.h) in numpy: per element the finite
    samples of the entering channels sorted by integer key and indexed.  ``cube`` float32
    [C][...plane]; ``filled`` [C].  Returns ``{name: [...plane]}`` for all five maps ('count' int32),
    or with ``subtract`` ``(maps, line)``, ``line`` a new array: the cube's own values in the channels
    that are not filled."""
    if not isinstance(params, SpectrumStatsParameters):
        raise TypeError('params must be SpectrumStatsParameters')
    cube = host_cube(cube)
    C = cube.shape[0]
    plane = cube.shape[1:]
    enter = params.entering(C, filled)
    filled = np.asarray(filled) != 0
    x = cube[enter].reshape(int(enter.sum()), int(np.prod(plane)))
    sample = np.isfinite(x)
    n = sample.sum(axis=0).astype(np.int64)
    by_value = np.sort(np.where(sample, keys(x).astype(np.uint64), _NONE), axis=0)
    median = _middle(by_value, n)
    nan = np.float32(np.nan)
    if x.shape[0]:
        low = values_of((by_value[0] & np.uint64(0xffffffff)).astype(np.uint32))
        top = np.take_along_axis(by_value, np.maximum(n - 1, 0)[np.newaxis], 0)[0]
        high = values_of((top & np.uint64(0xffffffff)).astype(np.uint32))
    else:
        low = high = np.full(n.shape, nan, np.float32)
    with np.errstate(all='ignore'):
        v = x if params.estimator == 'median_abs' else (x - median[np.newaxis]).astype(np.float32)
        spread = np.ascontiguousarray(v, np.float32).view(np.uint32) & np.uint32(0x7fffffff)
        by_spread = np.sort(np.where(sample, keys(spread.view(np.float32)).astype(np.uint64), _NONE), axis=0)
        sigma = (_middle(by_spread, n) * TO_RMS).astype(np.float32)
    enough = n >= params.min_samples
    maps = {
        'median': np.where(enough, median, nan).astype(np.float32).reshape(plane),
        'sigma': np.where(enough, sigma, nan).astype(np.float32).reshape(plane),
        'min': np.where(enough, low, nan).astype(np.float32).reshape(plane),
        'max': np.where(enough, high, nan).astype(np.float32).reshape(plane),
        'count': n.astype(np.int32).reshape(plane),
    }
    if not subtract:
        return maps
    line = cube.copy()
    with np.errstate(all='ignore'):
        for c in range(C):
            if filled[c]:
                line[c] = np.where(enough.reshape(plane), (cube[c] - maps['median']).astype(np.float32), nan)
    return maps, line


def resident_limit():
    """The largest number of entering channels the resident form takes."""
    return int(lib().kimg_spectrum_stats_resident_limit())


class SpectrumStats(CubeOperator):
    """``kimg_spectrum_stats`` for cubes of shape ``cube_shape`` = (C, P, H, W).  ``op(the_cube,
    subtract=False, out=None)`` takes a :class:`cube.SpectralCube` and returns ``{name: MapArray
    [P][H][W]}`` for the parameters' ``outputs`` ('count' int32, the others float32); maps that were
    not asked for are not returned.  With ``subtract=True`` the median is taken out of every filled
    channel, in place or into ``out``, another SpectralCube of the same shape and frequencies, which
    gets the input's ``filled`` and ``noise``.  The call is asynchronous on ``command_queue``.

    ``op(array, filled=..., subtract=..., out=array2)`` takes plain :class:`accel.DeviceArray`
    [C][P][H][W] instead, whose [P][H][W] plane is dense while the channel axis may have any pitch,
    each array its own; ``out`` must be the array itself (or None: in place) or share no memory with
    it."""

    def __init__(self, template, command_queue, cube_shape):
        super().__init__(template, command_queue, cube_shape)
        self.range = self.params.range(self.cube_shape[0])
        self._stat = self.params.stat(self.cube_shape[0])

    def __call__(self, cube, filled=None, subtract=False, out=None):
        params = self.params
        C = self.cube_shape[0]
        if not is_bool(subtract):
            raise ValueError('subtract must be a bool')
        if out is not None and not subtract:
            raise ValueError('out is where subtract=True writes; it was not asked for')
        array = self._array(cube, 'cube')
        filled = self._own_filled(cube, filled)
        check_out_cube(cube, out, 'line cube')
        filled = self._filled(filled)
        pitch = channel_pitch(array)
        target = target_pitch = None
        if subtract:
            target = array if out is None else self._array(out, 'out')
            target_pitch = channel_pitch(target)
        queue = self.command_queue
        context = queue.context
        plane = self.cube_shape[1:]
        # (the subtraction reads the median map, asked for or not)
        names = list(params.outputs)
        if subtract and 'median' not in names:
            names.append('median')
        maps = {name: MapArray(context, plane, np.int32 if name == 'count' else np.float32, queue=queue)
                for name in names}
        bits = 0
        for name in maps:
            bits |= OUTPUT_BITS[name]
        array.used_on(queue)
        if target is not None:
            target.used_on(queue)
        pointers = [maps[name].ptr if name in maps else None
                    for name in ('median', 'sigma', 'min', 'max', 'count')]
        first, stop = self.range
        check(lib().kimg_spectrum_stats(
            array.ptr, pitch, C, int(np.prod(plane)), first, stop,
            self._stat.ctypes.data_as(ctypes.c_void_p), filled.ctypes.data_as(ctypes.c_void_p),
            ESTIMATORS[params.estimator], params.min_samples, bits, *pointers,
            None if target is None else target.ptr, 0 if target is None else target_pitch,
            FORMS[self.template.form], queue.handle), 'kimg_spectrum_stats')
        mark_ready(queue, maps.values())
        carry_over(cube, out)
        return {name: maps[name] for name in params.outputs}


class SpectrumStatsTemplate(OperatorTemplate):
    """``tuning``: None or ``{'form': 'auto' | 'resident' | 'streaming'}`` -- the kernel form
    (csrc/spectrum_stats.hip); 'resident' takes at most :func:`resident_limit` entering channels."""

    params_type = SpectrumStatsParameters
    operator = SpectrumStats

    def __init__(self, context, params, tuning=None):
        super().__init__(context, params)
        tuning = dict(tuning or {})
        self.form = tuning.pop('form', 'auto')
        if tuning or self.form not in FORMS:
            raise ValueError("tuning must be {'form': 'auto', 'resident' or 'streaming'}")
