"""Phase-centre shift: raw visibilities re-phased to another direction and their baseline
coordinates rotated into that direction's frame (CASA's ``phaseshift`` / ``fixvis``, WSClean's
``chgcentre``, MIRIAD's ``uvedit``), on raw blocks, ahead of the continuum fit and of preprocessing.

The reference images around the phase centre of the observation and has no such step; a line target
off axis then costs an image wide enough to contain it, and the uv-plane continuum fit
(:mod:`.continuum`) is exact only for a source at the phase centre.  The contract is written in
include/kimg.h ("Phase-centre shift"); :func:`phase_shift_host` is the same contract as numpy, and
the executable specification the device (csrc/phaseshift.hip, :class:`PhaseShift`) is tested
against.  ``loader.preprocess_visibilities(..., phase_centre=(ra, dec))`` puts the operator between
the loader and the collector, ``continuum_centre=(ra, dec)`` around the continuum fit.

Feed angles are not recomputed for the new centre: valid for shifts small against a radian.
"""
import ctypes
import math

import numpy as np

from . import accel
from ._lib import lib, check
from .channel_block import ChannelOperator, OperatorTemplate, channel_pitch

LIGHTSPEED = 299792458.0


def frame(ra, dec):
    """float64 [3][3]: the rows e_u, e_v, e_w of the frame of direction (ra, dec), radians."""
    sa, ca = math.sin(ra), math.cos(ra)
    sd, cd = math.sin(dec), math.cos(dec)
    return np.array([[-sa, ca, 0.0],
                     [-sd * ca, -sd * sa, cd],
                     [cd * ca, cd * sa, sd]], np.float64)


def _lmn_minus_pole(centre, direction):
    """(l, m, n - 1, n) of ``direction`` in the frame of ``centre``, from the differences of the
    angles, so that a small shift keeps its digits: with a = ra' - ra, h = sin^2(a / 2),
    l = cos dec' sin a, m = sin(dec' - dec) + 2 cos dec' sin dec h and
    n = cos(dec' - dec) - 2 cos dec' cos dec h; n - 1 = -(l^2 + m^2) / (1 + n)."""
    (ra0, dec0), (ra, dec) = centre, direction
    a = ra - ra0
    h = math.sin(0.5 * a) ** 2
    l = math.cos(dec) * math.sin(a)
    m = math.sin(dec - dec0) + 2.0 * math.cos(dec) * math.sin(dec0) * h
    n = math.cos(dec - dec0) - 2.0 * math.cos(dec) * math.cos(dec0) * h
    if n <= 0.0:
        return l, m, n - 1.0, n
    return l, m, -(l * l + m * m) / (1.0 + n), n


def _centre(value, what):
    try:
        ra, dec = (float(x) for x in value)
    except (TypeError, ValueError):
        raise ValueError('{} must be (ra, dec) in radians'.format(what)) from None
    if not (math.isfinite(ra) and math.isfinite(dec)):
        raise ValueError('{} must be finite'.format(what))
    return ra, dec


class PhaseShiftParameters:
    """``frame_centre``: the direction (ra, dec), radians, whose frame the input uvw is in;
    ``new_centre``: the direction the visibilities are to be phased to, and whose frame the output
    uvw is in; ``from_centre``: the direction they are phased to now (default: ``frame_centre``).
    The new centre, and ``from_centre``, must lie less than 90 degrees from the frame centre.

    ``rotation`` [3][3]: uvw' = rotation . uvw (exactly the identity when ``new_centre`` equals
    ``frame_centre``).  ``lmn``: the new centre in the input frame (the third row of ``rotation``).
    ``delay`` [3]: lmn(new) - lmn(from) in the input frame, the pole's n - 1 taken without
    cancellation; the visibilities are multiplied by exp(+2 pi i delay . uvw / wavelength)."""

    def __init__(self, frame_centre, new_centre, from_centre=None):
        self.frame_centre = _centre(frame_centre, 'frame_centre')
        self.new_centre = _centre(new_centre, 'new_centre')
        self.from_centre = self.frame_centre if from_centre is None \
            else _centre(from_centre, 'from_centre')
        l1, m1, p1, n1 = _lmn_minus_pole(self.frame_centre, self.new_centre)
        l0, m0, p0, n0 = _lmn_minus_pole(self.frame_centre, self.from_centre)
        if n1 <= 0.0:
            raise ValueError('new_centre lies 90 degrees or more from frame_centre')
        if n0 <= 0.0:
            raise ValueError('from_centre lies 90 degrees or more from frame_centre')
        self.lmn = np.array([l1, m1, n1], np.float64)
        self.delay = np.array([l1 - l0, m1 - m0, p1 - p0], np.float64)
        if self.new_centre == self.frame_centre:
            self.rotation = np.identity(3, np.float64)
        else:
            self.rotation = frame(*self.new_centre) @ frame(*self.frame_centre).T

    @property
    def writes_uvw(self):
        """False when the output frame is the input frame (nothing to rotate)."""
        return self.new_centre != self.frame_centre

    def params12(self):
        """float64 [12]: ``rotation`` row by row, then ``delay`` (``kimg_phase_shift``)."""
        return np.concatenate((self.rotation.reshape(9), self.delay)).astype(np.float64)

    def __repr__(self):
        return 'PhaseShiftParameters({!r}, {!r}, from_centre={!r})'.format(
            self.frame_centre, self.new_centre, self.from_centre)


def offset_to_radec(centre, l, m):
    """(ra, dec) of the direction at direction cosines (l, m) in the frame of ``centre``."""
    n = math.sqrt(1.0 - l * l - m * m)
    x, y, z = frame(*_centre(centre, 'centre')).T @ np.array([l, m, n])
    return math.atan2(y, x), math.asin(max(-1.0, min(1.0, z)))


def inverse_wavelengths(frequencies):
    """float64 [C]: f / c0, the ``inv_wavelength`` argument."""
    return np.atleast_1d(np.asarray(frequencies, np.float64)) / LIGHTSPEED


def phase_shift_host_double(vis, uvw, inv_wavelength, params):
    """The contract up to its last step: (vis complex128 [C][N][Q] BEFORE the one rounding to
    complex64 the contract allows, uvw' float64 [N][3])."""
    vis = np.asarray(vis)
    uvw = np.asarray(uvw)
    if vis.dtype != np.complex64 or uvw.dtype != np.float32:
        raise TypeError('vis must be complex64 and uvw float32')
    if vis.ndim != 3 or uvw.shape != (vis.shape[1], 3):
        raise ValueError('vis must be [channel][row][polarization] and uvw [row][3]')
    inv_wavelength = np.asarray(inv_wavelength, np.float64)
    if inv_wavelength.shape != (vis.shape[0],):
        raise ValueError('one inverse wavelength per channel')
    x = uvw.astype(np.float64)
    R, delay = params.rotation, params.delay
    with np.errstate(all='ignore'):
        new_uvw = np.stack([(R[i, 0] * x[:, 0] + R[i, 1] * x[:, 1]) + R[i, 2] * x[:, 2]
                            for i in range(3)], axis=1)
        d = (delay[0] * x[:, 0] + delay[1] * x[:, 1]) + delay[2] * x[:, 2]
        turns = inv_wavelength[:, np.newaxis] * d[np.newaxis, :]
        reduced = turns - np.rint(turns)
        angle = 2.0 * np.pi * reduced
        c, s = np.cos(angle)[:, :, np.newaxis], np.sin(angle)[:, :, np.newaxis]
        re, im = vis.real.astype(np.float64), vis.imag.astype(np.float64)
        # (spelled out: numpy's complex product turns inf * (c + 0i) into NaN in places of its own)
        out = np.empty(vis.shape, np.complex128)
        out.real = re * c - im * s
        out.imag = re * s + im * c
    return out, new_uvw


def phase_shift_host(vis, uvw, inv_wavelength, params):
    """The contract of ``kimg_phase_shift`` (include/kimg.h) in numpy: float64 until the final
    rounding.  ``vis`` complex64 [C][N][Q], ``uvw`` float32 [N][3] in metres, ``inv_wavelength``
    float64 [C].  Returns new arrays (vis complex64, uvw' float32)."""
    out, new_uvw = phase_shift_host_double(vis, uvw, inv_wavelength, params)
    with np.errstate(all='ignore'):
        return out.astype(np.complex64), new_uvw.astype(np.float32)


class PhaseShift(ChannelOperator):
    """``kimg_phase_shift`` for blocks whose channels have the inverse wavelengths
    ``inv_wavelength`` (float64, 1 / metres; :func:`inverse_wavelengths`).  ``op(vis, uvw)`` rotates
    the visibilities of a :class:`accel.DeviceArray` [C][N][Q] (complex64; the [N][Q] plane dense,
    the channel axis of any pitch) in place and returns a new device array with the rotated
    coordinates of ``uvw`` (float32 [N][3], contiguous; left as it is), or, with
    ``write_uvw=False``, rotates the visibilities only and returns None.  Asynchronous on
    ``command_queue``."""

    COUNTERS = 0

    def __init__(self, template, command_queue, inv_wavelength):
        inv_wavelength = np.ascontiguousarray(np.atleast_1d(inv_wavelength), np.float64)
        if inv_wavelength.ndim != 1 or len(inv_wavelength) < 1 or not np.all(np.isfinite(inv_wavelength)):
            raise ValueError('inv_wavelength must be finite, one per channel')
        super().__init__(template, command_queue, len(inv_wavelength))
        self._params12 = np.ascontiguousarray(template.params.params12())
        self._inv_wavelength = accel.DeviceArray(command_queue.context, inv_wavelength.shape, np.float64,
                                                 queue=command_queue)
        self._inv_wavelength.set(command_queue, inv_wavelength)

    def __call__(self, vis, uvw, write_uvw=True):
        if vis.dtype != np.complex64 or uvw.dtype != np.float32:
            raise TypeError('vis must be complex64 and uvw float32')
        if len(vis.shape) != 3 or tuple(uvw.shape) != (vis.shape[1], 3):
            raise ValueError('vis must be [channel][row][polarization] and uvw [row][3]')
        self._check_channels(vis)
        if vis.shape[2] < 1:
            raise ValueError('no polarizations')
        if not uvw.tensor.is_contiguous():
            raise ValueError('uvw must be contiguous')
        queue = self.command_queue
        N = vis.shape[1]
        new_uvw = None
        if write_uvw:
            new_uvw = accel.DeviceArray(queue.context, (N, 3), np.float32, queue=queue)
        if N == 0:
            return new_uvw
        vis.used_on(queue)
        uvw.used_on(queue)
        check(lib().kimg_phase_shift(
            vis.ptr, channel_pitch(vis, 'vis'), self.num_channels, N, vis.shape[2], uvw.ptr,
            new_uvw.ptr if write_uvw else None, self._inv_wavelength.ptr,
            self._params12.ctypes.data_as(ctypes.c_void_p), queue.handle), 'kimg_phase_shift')
        return new_uvw


class PhaseShiftTemplate(OperatorTemplate):
    params_type = PhaseShiftParameters
    operator = PhaseShift
