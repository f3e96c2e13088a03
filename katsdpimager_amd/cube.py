"""The spectral cube and its moment maps: the images of a band's channels held in one device array
[channel][polarization][m][l], and that array reduced along the channel axis to the maps a
spectral-line user reads (CASA ``immoments``, MIRIAD ``moment``): integrated intensity (moment 0),
intensity-weighted coordinate (1, the velocity field), dispersion (2), peak (8) and coordinate of the
peak (9), each over the samples above a noise cut.

:class:`SpectralCube` is the container (it lives in :mod:`.cube_operator`, with what the cube
operators share, and is exported from here): ``frontend.process_channel`` leaves a channel's images in
the imager's buffers, :meth:`SpectralCube.put` copies one into its plane and records the channel's noise.
:class:`MomentsTemplate` / :class:`Moments` is the operator (csrc/moments.hip, ``kimg_moments``);
:func:`moments_host` is the same contract as numpy and the executable specification the device
matches bit for bit.

The contract (include/kimg.h, "Moment maps").  Every element m of the [P][H][W] plane on its own,
over the channels c = first .. stop - 1 in ascending order, I = cube[c][m]:

* I is usable iff ``filled[c]`` and I is finite.
* Selection value s = I, or with ``select_hanning`` s = ((0.25 a) + (0.5 I)) + (0.25 b) in float64,
  a and b the previous and next channel, each replaced by I itself where that channel is outside the
  range, not filled or not finite at m.
* The sample enters iff it is usable and ``(double) s > (double) cut[c]``; ``cut`` is float32 and made
  on the host: ``float32(clip_sigma) * noise[c]`` as a float32 product, the absolute ``cut``, or -inf.
* For each sample that enters, in float64 and unfused: ``n += 1; d = x[c] - x_ref; S0 += I;
  t = I * d; S1 += t; S2 += t * d``; the peak is replaced only if ``I > peak``, so the first channel
  wins a tie.  ``x_ref = x[(first + stop) // 2]``; ``width`` is the absolute mean spacing of x over the
  range, or, for a range of one channel, the cube's ``channel_width`` on the axis.
* Outputs, one rounding from float64 to float32 each: moment 0 = ``S0 * width``; 1 = ``x_ref + r``,
  ``r = S1 / S0``; 2 = ``sqrt(v)``, ``v = S2 / S0 - r * r`` with 0 in place of a negative v; 8 = the peak;
  9 = x of the peak's channel; ``count`` = n (int32).  Every moment is NaN where n == 0, moments 1 and 2
  also unless S0 > 0.  The cube is never written.

Not done: position-velocity cuts, cubes across several GPUs (with channels sharded over GPUs the
caller gathers planes with :meth:`SpectralCube.put`).  A selection smoothed in space and along the
spectrum is :mod:`.detect`'s smooth-and-clip mask, which :meth:`detect.MaskCube.apply` hands to
:class:`Moments` as NaN.  The median,
minimum and robust sigma along the spectrum (CASA moments 3 and 10) are :mod:`.spectrum_stats`'; still
missing are moments 4 to 7, the coordinate of the minimum (11) and a per-pixel cut made from those maps.  All planes share one pixel size, which is the caller's business; every
plane keeps its own restoring beam until :mod:`.smooth` takes the cube to a common one.  Image-plane
continuum subtraction on the cube is :mod:`.imcontsub`.  The noise :meth:`SpectralCube.put` records
is what the caller was told; :mod:`.cube_stats` measures it on the cube itself, for every plane in one
call, where nothing was told or the planes have changed since.
"""
import ctypes

import numpy as np

from . import accel
from ._lib import lib, check
from .channel_block import OperatorTemplate
# (the container and its helpers live with what the cube operators share; their old home exports them)
from .cube_operator import (  # noqa: F401
    AXES as _AXES, MAX_CHANNELS, SPEED_OF_LIGHT_KMS, CubeOperator, MapArray, SpectralCube,
    _rest_frequency, channel_pitch, channel_range, host_cube, host_filled, is_bool, mark_ready,
    range_in_band, velocities)

#: KIMG_MOMENT_* of include/kimg.h
MOMENT_BITS = {0: 1, 1: 2, 2: 4, 8: 8, 9: 16, 'count': 32}


def moment_bunit(moment, bunit='Jy/beam', axis='velocity'):
    """The FITS ``BUNIT`` of a moment map of a cube in ``bunit`` (for ``io.write_fits_image``)."""
    unit = {'velocity': 'km/s', 'frequency': 'Hz'}[axis]
    if moment == 0:
        return '{}.{}'.format(bunit, unit)
    if moment in (1, 2, 9):
        return unit
    if moment == 8:
        return bunit
    raise ValueError('no moment {!r}'.format(moment))


class MomentParameters:
    """``moments``: a subset of {0, 1, 2, 8, 9} (CASA's numbers: integrated, intensity-weighted
    coordinate, dispersion, peak, coordinate of the peak).  ``axis``: 'velocity' (radio convention,
    km/s, needs ``rest_frequency`` in Hz when the coordinates come from a :class:`SpectralCube`) or
    'frequency' (Hz).  ``channels`` = (first, stop), default the whole band.  At most one of
    ``clip_sigma`` (multiples of every channel's recorded noise) and ``cut`` (absolute, in the image's
    unit); with neither, everything finite enters.  ``select_hanning``: the cut is applied to the
    Hanning-smoothed spectrum, the sums still take the samples themselves."""

    def __init__(self, moments=(0, 1, 2), axis='velocity', rest_frequency=None, channels=None,
                 clip_sigma=None, cut=None, select_hanning=False):
        try:
            moments = tuple(moments)
        except TypeError:
            raise ValueError('moments must be a sequence') from None
        if not moments:
            raise ValueError('no moments asked for')
        for m in moments:
            if is_bool(m) or not isinstance(m, (int, np.integer)) \
                    or int(m) not in (0, 1, 2, 8, 9):
                raise ValueError('moments must come from 0, 1, 2, 8, 9, not {!r}'.format(m))
        moments = tuple(int(m) for m in moments)
        if len(set(moments)) != len(moments):
            raise ValueError('a moment is listed twice')
        self.moments = tuple(sorted(moments))
        if axis not in _AXES:
            raise ValueError("axis must be 'velocity' or 'frequency'")
        self.axis = axis
        self.rest_frequency = None if rest_frequency is None else _rest_frequency(rest_frequency)
        self.channels = None if channels is None else channel_range(channels, 'channels')
        if clip_sigma is not None and cut is not None:
            raise ValueError('at most one of clip_sigma and cut may be given')
        self.clip_sigma = None if clip_sigma is None else self._number(clip_sigma, 'clip_sigma')
        self.cut = None if cut is None else self._number(cut, 'cut')
        if not is_bool(select_hanning):
            raise ValueError('select_hanning must be a bool')
        self.select_hanning = bool(select_hanning)

    @staticmethod
    def _number(value, name):
        try:
            value = float(value)
        except (TypeError, ValueError):
            raise ValueError('{} must be a number'.format(name)) from None
        if value != value:
            raise ValueError('{} must not be NaN'.format(name))
        return value

    def range(self, num_channels):
        """(first, stop) within a band of ``num_channels`` channels."""
        return range_in_band(self.channels, num_channels)

    def cut_table(self, num_channels, noise=None, filled=None):
        """float32 [C]: the cut of every channel.  ``clip_sigma`` needs ``noise`` (float32 [C], NaN =
        none recorded) for every filled channel of the range."""
        first, stop = self.range(num_channels)
        if self.clip_sigma is not None:
            if noise is None:
                raise ValueError('clip_sigma needs the noise of every channel')
            noise = np.asarray(noise, np.float32)
            if noise.shape != (num_channels,):
                raise ValueError('noise must have one entry per channel')
            used = np.ones(stop - first, bool) if filled is None else np.asarray(filled)[first:stop] != 0
            if np.isnan(noise[first:stop][used]).any():
                raise ValueError('clip_sigma: a channel of the range has no noise recorded')
            with np.errstate(all='ignore'):
                return np.float32(self.clip_sigma) * noise
        value = -np.inf if self.cut is None else self.cut
        with np.errstate(over='ignore'):
            return np.full(num_channels, value, np.float32)

    def __repr__(self):
        text = 'MomentParameters({!r}, axis={!r}'.format(self.moments, self.axis)
        if self.rest_frequency is not None:
            text += ', rest_frequency={!r}'.format(self.rest_frequency)
        if self.channels is not None:
            text += ', channels={!r}'.format(self.channels)
        if self.clip_sigma is not None:
            text += ', clip_sigma={!r}'.format(self.clip_sigma)
        if self.cut is not None:
            text += ', cut={!r}'.format(self.cut)
        if self.select_hanning:
            text += ', select_hanning=True'
        return text + ')'


def range_width(x, first, stop, channel_width=None):
    """``width`` of the contract: the absolute mean spacing of ``x`` over first .. stop - 1, or
    ``|channel_width|`` (already on the axis of x) for a range of one channel."""
    if stop - first > 1:
        return float(abs(x[stop - 1] - x[first]) / np.float64(stop - first - 1))
    if channel_width is None:
        raise ValueError('a range of one channel needs the channel width')
    width = abs(float(channel_width))
    if width != width:
        raise ValueError('the channel width is NaN')
    return width


def _tables(num_channels, coordinates, cut, filled):
    x = np.ascontiguousarray(coordinates, np.float64)
    cut = np.ascontiguousarray(cut, np.float32)
    for name, table in (('coordinates', x), ('cut', cut)):
        if table.shape != (num_channels,):
            raise ValueError('{} must have one entry per channel'.format(name))
    return x, cut, host_filled(filled, num_channels).view(np.uint8)


def moments_host(cube, coordinates, cut, filled, params, channel_width=None):
    """The contract of ``kimg_moments`` (include/kimg.h) in numpy, float64 throughout and every sum in
    ascending channel order.  ``cube`` float32 [C][...plane]; ``coordinates`` float64 [C] (x);
    ``cut`` float32 [C]; ``filled`` [C]; ``channel_width`` on the axis of x, for a range of one
    channel.  Returns ``{moment: float32 [...plane]}`` for ``params.moments`` plus ``'count'`` (int32)."""
    cube = host_cube(cube)
    C = cube.shape[0]
    plane = cube.shape[1:]
    x, cut, filled = _tables(C, coordinates, cut, filled)
    first, stop = params.range(C)
    x_ref = x[(first + stop) // 2]
    width = np.float64(range_width(x, first, stop, channel_width))
    nan = np.full(plane, np.nan, np.float32)

    def neighbour(c, I):
        """channel c where it can stand next to I, else I itself (the replicate rule)"""
        if not first <= c < stop or not filled[c]:
            return I
        return np.where(np.isfinite(cube[c]), cube[c], I)
    n = np.zeros(plane, np.int32)
    S0 = np.zeros(plane, np.float64)
    S1 = np.zeros(plane, np.float64)
    S2 = np.zeros(plane, np.float64)
    peak = np.full(plane, -np.inf, np.float32)
    peak_channel = np.full(plane, first, np.int64)
    with np.errstate(all='ignore'):
        for c in range(first, stop):
            if not filled[c]:
                continue
            I = cube[c]
            Id = I.astype(np.float64)
            if params.select_hanning:
                a = neighbour(c - 1, I).astype(np.float64)
                b = neighbour(c + 1, I).astype(np.float64)
                s = ((0.25 * a) + (0.5 * Id)) + (0.25 * b)
            else:
                s = Id
            enter = np.isfinite(I) & (s > np.float64(cut[c]))
            d = x[c] - x_ref
            n = n + enter
            S0 = np.where(enter, S0 + Id, S0)
            t = Id * d
            S1 = np.where(enter, S1 + t, S1)
            S2 = np.where(enter, S2 + t * d, S2)
            higher = enter & (I > peak)
            peak = np.where(higher, I, peak)
            peak_channel = np.where(higher, c, peak_channel)
        some = n > 0
        positive = some & (S0 > 0)
        r = S1 / S0
        v = S2 / S0 - r * r
        v = np.where(v < 0, 0.0, v)
        values = {
            0: np.where(some, (S0 * width).astype(np.float32), nan),
            1: np.where(positive, (x_ref + r).astype(np.float32), nan),
            2: np.where(positive, np.sqrt(v).astype(np.float32), nan),
            8: np.where(some, peak, nan),
            9: np.where(some, x[peak_channel].astype(np.float32), nan),
        }
    out = {m: values[m].astype(np.float32) for m in params.moments}
    out['count'] = n.astype(np.int32)
    return out


class Moments(CubeOperator):
    """``kimg_moments`` for cubes of shape ``cube_shape`` = (C, P, H, W).  ``op(cube)`` takes a
    :class:`SpectralCube` and returns ``{moment: MapArray float32 [P][H][W]}`` for the moments of
    the parameters plus ``'count'`` (int32 [P][H][W], the samples that entered); maps that were not
    asked for are not allocated.  The call is asynchronous on ``command_queue`` once the per-channel
    tables (12 bytes a channel) are on the device; the cube is never written.

    ``op(array, coordinates=x, cut=cut, filled=filled)`` takes a plain :class:`accel.DeviceArray`
    [C][P][H][W] instead, whose [P][H][W] plane is dense while the channel axis may have any pitch (a
    view of a larger tensor): ``coordinates`` float64 [C], ``filled`` [C], and ``cut`` a float32 [C]
    table, one number, or None for what the parameters say (``clip_sigma`` needs a cube's noise and is
    refused here).  ``channel_width``, on the axis of x, serves a range of one channel."""

    def __init__(self, template, command_queue, cube_shape):
        super().__init__(template, command_queue, cube_shape)
        self.range = self.params.range(self.cube_shape[0])
        self._tables = None

    def __call__(self, cube, coordinates=None, cut=None, filled=None, channel_width=None):
        params = self.params
        C = self.cube_shape[0]
        first, stop = self.range
        array = self._array(cube, 'cube')
        filled = self._own_filled(cube, filled, coordinates=coordinates, cut=cut,
                                  channel_width=channel_width)
        if isinstance(cube, SpectralCube):
            coordinates = cube.coordinates(params.axis, params.rest_frequency)
            cut = params.cut_table(C, cube.noise, filled)
            if stop - first == 1:
                channel_width = cube.axis_channel_width(params.axis, params.rest_frequency)
        else:
            if coordinates is None:
                raise ValueError('a plain array needs coordinates')
            if cut is None:
                cut = params.cut_table(C)
            elif np.ndim(cut) == 0:
                cut = np.full(C, MomentParameters._number(cut, 'cut'), np.float32)
        x, cut, filled = _tables(C, coordinates, cut, filled)
        width = range_width(x, first, stop, channel_width)
        pitch = channel_pitch(array)
        queue = self.command_queue
        context = queue.context
        # one upload: x, then cut
        tables = np.concatenate((x.view(np.uint8), cut.view(np.uint8)))
        if self._tables is None or self._tables.shape != tables.shape:
            self._tables = accel.DeviceArray(context, tables.shape, np.uint8, queue=queue)
        self._tables.set(queue, tables)
        plane = self.cube_shape[1:]
        out = {m: MapArray(context, plane, np.float32, queue=queue) for m in params.moments}
        out['count'] = MapArray(context, plane, np.int32, queue=queue)
        outputs = 0
        for key in out:
            outputs |= MOMENT_BITS[key]
        array.used_on(queue)
        pointers = [out[m].ptr if m in out else None for m in (0, 1, 2, 8, 9, 'count')]
        check(lib().kimg_moments(
            array.ptr, pitch, C, int(np.prod(plane)), first, stop, self._tables.ptr,
            self._tables.ptr + 8 * C, filled.ctypes.data_as(ctypes.c_void_p), width,
            int(params.select_hanning), outputs, *pointers, queue.handle), 'kimg_moments')
        mark_ready(queue, out.values())
        return out


class MomentsTemplate(OperatorTemplate):
    params_type = MomentParameters
    operator = Moments

