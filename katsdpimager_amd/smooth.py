"""Cube smoothing to a common restoring beam: every plane of a spectral cube keeps the beam it was
restored with, which scales with ``1 / f`` -- and a Jy/beam value with the beam's area -- so a
pixel does not mean the same in every channel, which :mod:`.cube`'s moments and :mod:`.imcontsub`
assume.  This module makes it so (CASA ``imsmooth(targetres=True)`` / ``commonbeam``, MIRIAD
``convol options=final``): :func:`common_beam` chooses the beam every plane can be taken to,
:func:`kernel_tables` makes the small Gaussian kernel that takes each plane there, and
:class:`CubeSmoothTemplate` / :class:`CubeSmooth` convolve all planes with theirs in one launch
(csrc/cube_smooth.hip, ``kimg_cube_smooth``).  :func:`cube_smooth_host` is the convolution's contract
as numpy, the executable specification the device matches bit for bit.

The contract is written in include/kimg.h ("Cube smoothing to a common beam").  Beams are
:class:`beam.Beam` objects in pixels, as ``beam.fit_beam`` returns them: x is axis 0 and the
covariance is ``Sigma = M M^T``, ``M = beam.beam_covariance_sqrt(beam)``.  The kernel of channel c
has the covariance ``Sigma_T - Sigma_c``, a fraction of a pixel to a few pixels over a spectral-line
band, so the convolution is direct (a footprint of up to 33 x 33), not ``beam.ConvolveBeam``'s two
transforms a plane.  The direct form is the faster one for small kernels only: its time grows with
the number of taps, and on one MI355X ``beam.ConvolveBeam`` plane by plane overtakes
it from a radius of about 6; radii up to 16 are taken so that the odd wide channel of a cube does
not need a second route, but a cube whose kernels are mostly wider than 6 px in radius (``truncate``
times a sigma of 1.5 px) is better served there.

The noise of a smoothed plane is correlated from pixel to pixel and lower than the input's by an
amount that depends on the noise's own correlation; it is not derived here.  The returned cube's
``noise`` is the input's times the flux factor where a plane was only scaled (``R = 0``) and NaN
elsewhere: the caller measures it again (``frontend.process_channel``'s estimate on the smoothed
plane) or sets it before anything that needs it (``clip_sigma``, ``weighting='noise'``).
:mod:`.cube_stats` measures it on the returned cube, all planes in one call
(``op(smoothed, update_noise=True)``).

Not done: minimum-area common beams of differently shaped ellipses (:func:`common_beam` scales the
largest beam until it contains the others), kernels beyond ``R = 16`` (``beam.ConvolveBeam``'s
work), sub-pixel kernels sampled better than at pixel centres, the noise of the smoothed planes,
in-place operation, cubes across several GPUs.
"""
import ctypes
import math

import numpy as np

from . import accel
from ._lib import lib, check
from .beam import Beam, beam_covariance_sqrt
from .cube_operator import (  # noqa: F401  (MAX_CHANNELS: the limit band_size holds this module to)
    MAX_CHANNELS, CubeOperator, CubeTemplate, SpectralCube, band_size, blank_stale_planes, channel_pitch,
    check_out_cube, host_cube)

#: KIMG_CUBE_SMOOTH_MAX_RADIUS
MAX_RADIUS = 16
#: entries of a channel's row of the taps table
TAPS_PITCH = (2 * MAX_RADIUS + 1) ** 2
#: below this sigma (pixels) a kernel is the identity: the plane is only scaled
MIN_SIGMA = 0.05
#: the floor of a kernel's eigenvalues, (1e-3 px)^2
_FLOOR = 1e-6
#: an eigenvalue of Sigma_T - Sigma_c below -_CONTAINS * trace(Sigma_T): T does not contain c
_CONTAINS = 1e-9

_UNITS = ('beam', 'pixel')


def beam_covariance(beam):
    """``Sigma = M M^T`` of a :class:`beam.Beam`, float64 [2][2], pixels^2, x = axis 0."""
    M = np.asarray(beam_covariance_sqrt(beam), np.float64)
    return M @ M.T


def _det(sigma):
    return float(sigma[0, 0] * sigma[1, 1] - sigma[0, 1] * sigma[1, 0])


def _filled_beams(beams, filled):
    beams = list(beams)
    if filled is None:
        filled = [b is not None for b in beams]
    filled = np.asarray(filled) != 0
    if filled.shape != (len(beams),):
        raise ValueError('filled must have one entry per beam')
    for c in np.flatnonzero(filled):
        if not isinstance(beams[c], Beam):
            raise ValueError('channel {} is filled and has no beam'.format(int(c)))
    return beams, filled


def common_beam(beams, filled=None):
    """The smallest scaled copy of the largest beam that contains every beam, exactly: with L the
    beam of largest area ``sqrt(det Sigma)`` (the lowest channel of a tie), ``s Sigma_L`` with
    ``s = max_c lambda_max(Sigma_L^-1/2 Sigma_c Sigma_L^-1/2)``, as a :class:`beam.Beam`.  For
    beams of one shape that scale with frequency this is the largest beam itself.  Host, float64.
    ``beams``: one per channel (None where ``filled``, default "has a beam", is 0)."""
    beams, filled = _filled_beams(beams, filled)
    channels = [int(c) for c in np.flatnonzero(filled)]
    if not channels:
        raise ValueError('no beam to choose from')
    sigma = {c: beam_covariance(beams[c]) for c in channels}
    area = {c: math.sqrt(max(_det(sigma[c]), 0.0)) for c in channels}
    L = channels[0]
    for c in channels:
        if area[c] > area[L]:
            L = c
    value, vector = np.linalg.eigh(sigma[L])
    if value[0] <= 0.0:
        raise ValueError('the beam of channel {} is degenerate'.format(L))
    inverse_root = vector @ np.diag(1.0 / np.sqrt(value)) @ vector.T
    s = 1.0
    for c in channels:
        if c != L:
            s = max(s, float(np.linalg.eigvalsh(inverse_root @ sigma[c] @ inverse_root.T)[1]))
    model = beams[L].model
    root = math.sqrt(s)
    return Beam(1.0, model.x_stddev.value * root, model.y_stddev.value * root, float(model.theta))


def kernel_radius(sigma_max, truncate=4.0):
    """``R`` of a kernel whose larger sigma is ``sigma_max`` pixels: 0 below 0.05 px, else
    ``ceil(truncate * sigma_max)``."""
    if sigma_max < MIN_SIGMA:
        return 0
    return int(math.ceil(truncate * sigma_max))


def _truncate(value):
    try:
        value = float(value)
    except (TypeError, ValueError):
        raise ValueError('truncate must be a number') from None
    if not 0.0 < value < np.inf:
        raise ValueError('truncate must be finite and above 0')
    return value


def _kernels(beams, target, filled, truncate, units):
    """Per filled channel: (Sigma_K's floored eigenvalues and its eigenvectors, R, flux factor).
    ``truncate`` None: no radius is worked out (R is None) and none refused -- the flux factor does
    not depend on it."""
    if truncate is not None:
        truncate = _truncate(truncate)
    if units not in _UNITS:
        raise ValueError("units must be 'beam' or 'pixel'")
    if not isinstance(target, Beam):
        raise TypeError('target must be a Beam')
    beams, filled = _filled_beams(beams, filled)
    band_size(len(beams))
    sigma_t = beam_covariance(target)
    det_t = _det(sigma_t)
    out = {}
    for c in (int(c) for c in np.flatnonzero(filled)):
        sigma_c = beam_covariance(beams[c])
        value, vector = np.linalg.eigh(sigma_t - sigma_c)
        if value[0] < -_CONTAINS * float(np.trace(sigma_t)):
            raise ValueError('the target does not contain the beam of channel {}'.format(c))
        value = np.maximum(value, _FLOOR)
        R = None if truncate is None else kernel_radius(math.sqrt(float(value[1])), truncate)
        if R is not None and R > MAX_RADIUS:
            raise ValueError('channel {} needs a kernel of radius {} > {}: such a plane is work for '
                             'beam.ConvolveBeam'.format(c, R, MAX_RADIUS))
        det_c = _det(sigma_c)
        if not det_c > 0.0:
            raise ValueError('the beam of channel {} is degenerate'.format(c))
        factor = math.sqrt(det_t / det_c) if units == 'beam' else 1.0
        out[c] = (value, vector, R, factor)
    return len(beams), out


def flux_factors(beams, target, filled=None, units='beam'):
    """float64 [C]: what a plane is multiplied by on top of the unit-sum kernel -- the ratio of the
    beam areas ``sqrt(det Sigma_T / det Sigma_c)`` for Jy/beam, 1 for ``units='pixel'``; NaN for a
    channel that is not filled.  It depends neither on ``truncate`` nor on a kernel's radius: of
    :func:`kernel_tables`' refusals it has the missing beam and the target that does not contain a
    beam, not ``R > 16``."""
    C, kernels = _kernels(beams, target, filled, None, units)
    factors = np.full(C, np.nan)
    for c, (_, _, _, factor) in kernels.items():
        factors[c] = factor
    return factors


def kernel_tables(beams, target, filled=None, truncate=4.0, units='beam'):
    """``(radius int32 [C], taps float32 [C][33 * 33])``: per filled channel the Gaussian of
    covariance ``Sigma_K = Sigma_T - Sigma_c`` sampled at pixel centres over ``[-R, R]^2``,
    ``R = kernel_radius(sigma_max, truncate)``, divided by its sum (float64, row-major order),
    multiplied by the flux factor (:func:`flux_factors`) and rounded once to float32; channel c uses
    the first ``(2 R + 1)^2`` entries of its row, row-major ``[dy][dx]`` with y = axis 0.  Eigenvalues
    of ``Sigma_K`` are floored at (1e-3 px)^2.  ValueError for a filled channel without a beam, for
    a target that does not contain a channel's beam (an eigenvalue below ``-1e-9 trace(Sigma_T)``)
    and for ``R > 16``.  Host, float64."""
    C, kernels = _kernels(beams, target, filled, truncate, units)
    radius = np.zeros(C, np.int32)
    taps = np.zeros((C, TAPS_PITCH), np.float32)
    for c, (value, vector, R, factor) in kernels.items():
        inverse = vector @ np.diag(1.0 / value) @ vector.T
        d = np.arange(-R, R + 1, dtype=np.float64)
        dy, dx = d[:, np.newaxis], d[np.newaxis, :]
        g = np.exp(-0.5 * (inverse[0, 0] * dy * dy + 2.0 * inverse[0, 1] * dy * dx
                           + inverse[1, 1] * dx * dx)).reshape(-1)
        total = 0.0
        for x in g:                 # (row-major, one by one: the order is part of the contract)
            total += x
        radius[c] = R
        taps[c, :g.size] = (g / total * factor).astype(np.float32)
    return radius, taps


def _check_tables(C, filled, radius, taps):
    filled = np.ascontiguousarray(np.asarray(filled) != 0, np.uint8)
    radius = np.ascontiguousarray(radius, np.int32)
    taps = np.asarray(taps)
    if taps.dtype != np.float32:
        raise TypeError('taps must be float32')
    taps = np.ascontiguousarray(taps)
    if filled.shape != (C,) or radius.shape != (C,) or taps.ndim != 2 or taps.shape[0] != C:
        raise ValueError('filled, radius and taps must have one entry per channel')
    for c in np.flatnonzero(filled):
        if not 0 <= radius[c] <= MAX_RADIUS:
            raise ValueError('radius {} of channel {} is outside 0 to {}'.format(radius[c], c, MAX_RADIUS))
        if (2 * int(radius[c]) + 1) ** 2 > taps.shape[1]:
            raise ValueError('the taps of channel {} do not fit the table'.format(c))
    return filled, radius, taps


def cube_smooth_host(cube, filled, radius, taps, out=None):
    """The contract of ``kimg_cube_smooth`` (include/kimg.h) in numpy.  ``cube`` float32
    [C][P][H][W]; ``filled`` [C]; ``radius`` int32 [C] and ``taps`` float32 [C][>= (2 R + 1)^2] as
    :func:`kernel_tables` makes them.  Every filled plane is padded with R zeros and, for dy
    ascending and within it dx ascending, ``acc = acc + (tap * shifted plane)`` in float32 from
    +0.0, every product and sum rounded; a NaN result is stored as 0x7fc00000.  Returns a new array
    whose unfilled channels are ``out``'s (NaN without one)."""
    cube = host_cube(cube, ndim=4)
    C, P, H, W = cube.shape
    filled, radius, taps = _check_tables(C, filled, radius, taps)
    result = np.full(cube.shape, np.nan, np.float32) if out is None else np.array(out, np.float32)
    if result.shape != cube.shape:
        raise ValueError('out has another shape')
    quiet = np.array([0x7fc00000], np.uint32).view(np.float32)[0]
    with np.errstate(all='ignore'):
        for c in np.flatnonzero(filled):
            R = int(radius[c])
            D = 2 * R + 1
            padded = np.zeros((P, H + 2 * R, W + 2 * R), np.float32)
            padded[:, R:R + H, R:R + W] = cube[c]
            acc = np.zeros((P, H, W), np.float32)
            for iy in range(D):
                for ix in range(D):
                    acc = acc + taps[c, iy * D + ix] * padded[:, iy:iy + H, ix:ix + W]
            result[c] = np.where(np.isnan(acc), quiet, acc)
    return result


class CommonBeamParameters:
    """``target``: the :class:`beam.Beam` (pixels) every plane is taken to, or None for
    :func:`common_beam` of the filled planes.  ``truncate``: a kernel reaches out to this many of
    its larger sigma.  ``units``: 'beam' for a cube in Jy/beam (a plane is scaled by the ratio of
    the beam areas on top of the convolution), 'pixel' for one in Jy/pixel (the sum of a plane is
    kept)."""

    def __init__(self, target=None, truncate=4.0, units='beam'):
        if target is not None and not isinstance(target, Beam):
            raise TypeError('target must be a Beam or None')
        self.target = target
        self.truncate = _truncate(truncate)
        if units not in _UNITS:
            raise ValueError("units must be 'beam' or 'pixel'")
        self.units = units

    def __repr__(self):
        return 'CommonBeamParameters(target={!r}, truncate={!r}, units={!r})'.format(
            self.target, self.truncate, self.units)


class CubeSmooth(CubeOperator):
    """``kimg_cube_smooth`` for cubes of shape ``cube_shape`` = (C, P, H, W).  ``op(cube)`` takes a
    :class:`cube.SpectralCube` whose planes were :meth:`~cube.SpectralCube.put` with their beams and
    returns a second SpectralCube, allocated unless ``out=`` gives one (same shape, frequencies,
    polarizations and channel width, not the cube itself): every filled plane smoothed to the
    target, ``common_beam`` and every filled plane's entry of ``beams`` set to the target,
    ``filled`` the source's, ``noise`` as the module's docstring says.  A given ``out`` is taken
    over whole: what it recorded of its planes is replaced, and a plane it held in a channel the
    source has not filled is set to NaN again, as in a fresh cube.  The source is never written.  The call is asynchronous on
    ``command_queue`` once the taps (4356 bytes a channel) are on the device.

    ``op(array, beams=..., filled=..., out=array2)`` takes plain :class:`accel.DeviceArray`
    [C][P][H][W] instead, whose [P][H][W] plane is dense while the channel axis may have any pitch,
    each array its own; ``out`` (allocated and filled with NaN when None) shares no memory with the
    array.  Returns ``out``.

    After a call ``target``, ``radius`` (int32 [C]) and ``factors`` (float64 [C]) say what it did."""

    def __init__(self, template, command_queue, cube_shape):
        super().__init__(template, command_queue, cube_shape, band=True)
        self.target = self.radius = self.factors = None
        self._taps = None

    def __call__(self, cube, out=None, beams=None, filled=None):
        params = self.params
        C = self.cube_shape[0]
        queue = self.command_queue
        context = queue.context
        from_cube = isinstance(cube, SpectralCube)
        array = self._array(cube, 'cube')
        filled = self._own_filled(cube, filled, beams=beams)
        if from_cube:
            beams = cube.beams
            if out is cube:
                raise ValueError('the smoothed cube cannot be the cube itself')
        elif beams is None:
            raise ValueError('a plain array needs beams')
        check_out_cube(cube, out, 'smoothed cube', same=('frequencies', 'polarizations', 'channel_width'))
        if out is not None:
            destination = self._array(out, 'out')
        beams, on = _filled_beams(beams, filled)
        if len(beams) != C:
            raise ValueError('beams must have one entry per channel')
        filled = np.ascontiguousarray(on, np.uint8)
        target = params.target
        if target is None:
            target = common_beam(beams, filled)
        radius, taps = kernel_tables(beams, target, filled, params.truncate, params.units)
        factors = flux_factors(beams, target, filled, params.units)
        # everything that can be refused has been: allocate
        if out is None:
            if from_cube:
                out = SpectralCube.like(cube, queue)
                destination = out.array
            else:
                out = destination = accel.DeviceArray(context, self.cube_shape, np.float32, queue=queue)
                check(lib().kimg_fill(out.ptr, int(np.prod(self.cube_shape)), float('nan'),
                                      queue.handle), 'kimg_fill')
        pitch = channel_pitch(array)
        out_pitch = channel_pitch(destination)
        if from_cube:
            blank_stale_planes(queue, destination, out_pitch, np.flatnonzero((out.filled != 0) & ~on),
                               int(np.prod(self.cube_shape[1:])))
        if self._taps is None:
            self._taps = accel.DeviceArray(context, taps.shape, np.float32, queue=queue)
        self._taps.set(queue, taps)
        array.used_on(queue)
        destination.used_on(queue)
        check(lib().kimg_cube_smooth(
            array.ptr, pitch, destination.ptr, out_pitch, *self.cube_shape,
            filled.ctypes.data_as(ctypes.c_void_p), radius.ctypes.data_as(ctypes.c_void_p),
            self._taps.ptr, taps.shape[1], queue.handle), 'kimg_cube_smooth')
        self.target, self.radius, self.factors = target, radius, factors
        if from_cube:
            scaled = np.float64(cube.noise) * np.where(on, factors, np.nan)
            out.filled[:] = filled
            out.noise[:] = np.where(on & (radius == 0), scaled, np.nan).astype(np.float32)
            out.beams = [target if f else None for f in on]
            out.common_beam = target
        return out


class CubeSmoothTemplate(CubeTemplate):
    params_type = CommonBeamParameters
    operator = CubeSmooth
