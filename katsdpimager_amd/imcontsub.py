"""Image-plane continuum subtraction: per pixel of a spectral cube, a low-order polynomial fitted
across the line-free channels and subtracted from every filled channel (CASA's ``imcontsub``,
MIRIAD's ``contsub``) -- the partner of :mod:`.continuum`, which does the same per baseline sample on
raw visibilities.  That route degrades away from the phase centre and needs the visibilities; this
one works on a cube that already exists, anywhere in the field, and is what keeps the continuum out
of moment 0.

The contract is written in include/kimg.h ("Image-plane continuum subtraction");
:func:`imcontsub_host` is the same contract as numpy, and the executable specification the device
(csrc/imcontsub.hip, :class:`ImContSub`) is tested against.  In short, for every element of the
[P][H][W] plane on its own: the channels that enter the fit are those of the selection that are
filled and carry a weight in (0, inf); a sample is usable iff it is finite; the normal equations are
summed in ascending channel order in float64 and solved by Cholesky without pivoting, all in the
steps of ``continuum.uvcontsub_host_double``; an element with ``n >= max(order + 1, min_samples)``
usable samples is fitted and has the model subtracted from every filled channel (non-finite samples
stay as they are), any other has its filled channels set to NaN.  Channels that are not filled are
neither read nor written.

Not done: robust polynomial fits and iterative clipping (the order-0 robust case, the per-pixel median
across the band that needs no line ranges, is :mod:`.spectrum_stats` with ``subtract=True``), per-pixel
weights, a fit across several cubes.
"""
import ctypes

import numpy as np

from . import accel
from ._lib import lib, check
from .channel_block import ChannelSelection, OperatorTemplate, integer
from .continuum import MAX_ORDER, legendre_basis
from .cube_operator import (MAX_CHANNELS, CubeOperator, MapArray, SpectralCube, band_size, carry_over,
                            channel_pitch, check_out_cube, host_cube, host_filled, mark_ready)

#: KIMG_IMCONTSUB_* of include/kimg.h
OUTPUT_BITS = {'continuum': 1, 'coefficients': 2, 'rms': 4, 'count': 8}
#: the maps of a call that does not say
DEFAULT_OUTPUTS = ('continuum', 'rms', 'count')
#: P_k(0), the Legendre polynomials at the middle of the axis
_MID_BAND = (1.0, 0.0, -0.5, 0.0)

_AXES = ('channel', 'frequency')
_WEIGHTINGS = ('none', 'noise')


class ImContSubParameters:
    """``order``: degree of the polynomial, 0 to 3.  Exactly one of ``fit_mask`` (one entry per
    channel, nonzero = a line-free channel) and ``line_ranges`` (a list of ``(first, last + 1)``
    channel ranges left OUT of the fit) says which channels are line-free.  ``axis``: the polynomial
    is one in channel index ('channel') or in the cube's frequencies ('frequency').  ``weighting``:
    'none' gives every channel the weight 1, 'noise' ``1 / noise[c]**2`` from the noise recorded with
    every plane, which every filled line-free channel must then have.  ``min_samples``: an element is
    fitted only with that many usable samples (never fewer than ``order + 1``); 1 to the number of
    channels.  At least ``order + 1`` channels must remain for the fit; what remains is known only
    once the cube is (:meth:`tables`)."""

    def __init__(self, order, fit_mask=None, line_ranges=None, axis='channel', weighting='none',
                 min_samples=None):
        try:
            as_int = int(order)
        except (TypeError, ValueError):
            raise ValueError('order must be an integer') from None
        if as_int != order or not 0 <= as_int <= MAX_ORDER:
            raise ValueError('order must be an integer from 0 to {}'.format(MAX_ORDER))
        self._selection = ChannelSelection(fit_mask, line_ranges, order=as_int)
        self.order = as_int
        self.fit_mask = self._selection.fit_mask
        self.line_ranges = self._selection.line_ranges
        if axis not in _AXES:
            raise ValueError("axis must be 'channel' or 'frequency'")
        self.axis = axis
        if weighting not in _WEIGHTINGS:
            raise ValueError("weighting must be 'none' or 'noise'")
        self.weighting = weighting
        self.min_samples = None
        if min_samples is not None:
            limit = MAX_CHANNELS if self.fit_mask is None else len(self.fit_mask)
            self.min_samples = integer(min_samples, 'min_samples', 1, max(limit, 1))
        if self.fit_mask is not None:
            self.mask(len(self.fit_mask))

    def mask(self, num_channels):
        """The selection over ``num_channels`` channels, uint8 (1 = line-free)."""
        num_channels = band_size(num_channels)
        if self.min_samples is not None and self.min_samples > num_channels:
            raise ValueError('min_samples {} for {} channels'.format(self.min_samples, num_channels))
        return self._selection.mask(num_channels)

    def basis(self, num_channels, frequencies=None):
        """float64 [order + 1][C]: ``continuum.legendre_basis`` by channel index, or with
        ``axis='frequency'`` by ``frequencies``, which are then needed."""
        if frequencies is not None:
            frequencies = np.asarray(frequencies, np.float64)
            if frequencies.shape != (num_channels,) or not np.all(np.isfinite(frequencies)):
                raise ValueError('frequencies must be finite, one per channel')
        if self.axis == 'channel':
            return legendre_basis(self.order, num_channels)
        if frequencies is None:
            raise ValueError("axis='frequency' needs the frequencies of the cube")
        return legendre_basis(self.order, num_channels, frequencies)

    def weights(self, num_channels, fit, noise=None):
        """float64 [C]: the weight of every channel; ``fit`` [C] says which channels would enter.
        'noise' needs ``noise`` (float32 [C], NaN = none recorded) for every one of those."""
        if self.weighting == 'none':
            return np.ones(num_channels, np.float64)
        if noise is None:
            raise ValueError("weighting='noise' needs the noise of every channel")
        noise = np.asarray(noise, np.float32)
        if noise.shape != (num_channels,):
            raise ValueError('noise must have one entry per channel')
        if np.isnan(noise[np.asarray(fit) != 0]).any():
            raise ValueError("weighting='noise': a filled line-free channel has no noise recorded")
        with np.errstate(all='ignore'):
            w = 1.0 / noise.astype(np.float64) ** 2
        return np.where(np.isnan(w), 0.0, w)

    def tables(self, num_channels, filled, frequencies=None, noise=None):
        """What a call is made of: ``(filled uint8 [C], fit uint8 [C] -- the channels that enter the
        fit: of the selection, filled, weight in (0, inf) --, w float64 [C], basis float64 [K][C],
        bref float64 [K], min_samples)``.  ValueError when fewer than ``order + 1`` channels enter."""
        C = int(num_channels)
        selection = self.mask(C)
        filled = host_filled(filled, C).view(np.uint8)
        B = self.basis(C, frequencies)
        asked = selection & filled
        w = self.weights(C, asked, noise)
        fit = np.ascontiguousarray(asked & (w > 0) & (w < np.inf), np.uint8)
        K = self.order + 1
        if int(fit.sum()) < K:
            raise ValueError('order {} needs {} filled, weighted line-free channels, {} remain'.format(
                self.order, K, int(fit.sum())))
        bref = np.array(_MID_BAND[:K], np.float64)
        return filled, fit, w, B, bref, 1 if self.min_samples is None else self.min_samples

    def __repr__(self):
        text = 'ImContSubParameters({!r}, {}'.format(self.order, self._selection.spelling())
        if self.axis != 'channel':
            text += ', axis={!r}'.format(self.axis)
        if self.weighting != 'none':
            text += ', weighting={!r}'.format(self.weighting)
        if self.min_samples is not None:
            text += ', min_samples={!r}'.format(self.min_samples)
        return text + ')'


def imcontsub_host_double(cube, filled, params, frequencies=None, noise=None):
    """The contract up to its last step: ``(line, maps)`` with every value in float64 BEFORE the one
    rounding to float32.  ``line`` [C][...plane]: the residual of fitted elements, NaN in the filled
    channels of the others, the input's own value where that is not finite or the channel not filled.
    ``maps``: ``'continuum'``, ``'coefficients'`` [K][...plane], ``'rms'`` (float64, NaN where the
    contract says so), ``'count'`` (int32) and ``'fitted'`` (bool)."""
    cube = host_cube(cube)
    C = cube.shape[0]
    plane = cube.shape[1:]
    filled, fit, w, B, bref, min_samples = params.tables(C, filled, frequencies, noise)
    K = params.order + 1
    A = np.zeros((K, K) + plane, np.float64)
    b = np.zeros((K,) + plane, np.float64)
    n = np.zeros(plane, np.int32)
    with np.errstate(all='ignore'):
        for c in range(C):
            if not fit[c]:
                continue
            usable = np.isfinite(cube[c])
            I = cube[c].astype(np.float64)
            n = n + usable
            for k in range(K):
                wb = w[c] * B[k, c]
                for l in range(k + 1):
                    A[k, l] = np.where(usable, A[k, l] + wb * B[l, c], A[k, l])
                b[k] = np.where(usable, b[k] + wb * I, b[k])
        fitted = n >= max(K, min_samples)
        # Cholesky A = L L^T without pivoting (lower triangle in place), L y = b, L^T a = y
        for k in range(K):
            for l in range(k + 1):
                s = A[k, l].copy()
                for i in range(l):
                    s -= A[k, i] * A[l, i]
                A[k, l] = np.sqrt(s) if l == k else s / A[l, l]
        a = np.zeros_like(b)
        for k in range(K):
            s = b[k].copy()
            for i in range(k):
                s -= A[k, i] * a[i]
            a[k] = s / A[k, k]
        for k in range(K - 1, -1, -1):
            s = a[k].copy()
            for i in range(k + 1, K):
                s -= A[i, k] * a[i]
            a[k] = s / A[k, k]
        line = cube.astype(np.float64)
        R = np.zeros(plane, np.float64)
        for c in range(C):
            if not filled[c]:
                continue
            model = np.zeros(plane, np.float64)
            for k in range(K):
                model += a[k] * B[k, c]
            usable = np.isfinite(cube[c])
            r = line[c] - model
            if fit[c]:
                R = np.where(usable, R + r * r, R)
            line[c] = np.where(fitted, np.where(usable, r, line[c]), np.nan)
        at_ref = np.zeros(plane, np.float64)
        for k in range(K):
            at_ref += a[k] * bref[k]
        rms = np.sqrt(R / (n - K).astype(np.float64))
    maps = {
        'continuum': np.where(fitted, at_ref, np.nan),
        'coefficients': np.where(fitted[np.newaxis], a, np.nan),
        'rms': np.where(fitted & (n > K), rms, np.nan),
        'count': n.astype(np.int32),
        'fitted': fitted,
    }
    return line, maps


def imcontsub_host(cube, filled, params, frequencies=None, noise=None):
    """The contract of ``kimg_imcontsub`` (include/kimg.h) in numpy: float64 until the one rounding
    to float32.  ``cube`` float32 [C][...plane], ``filled`` [C]; ``frequencies`` (float64 [C]) for
    ``axis='frequency'``, ``noise`` (float32 [C]) for ``weighting='noise'``.  Returns a new array and
    the maps: ``(line, {'continuum', 'coefficients', 'rms', 'count'})``."""
    cube = host_cube(cube)
    line, maps = imcontsub_host_double(cube, filled, params, frequencies, noise)
    with np.errstate(all='ignore'):
        rounded = line.astype(np.float32)
        out = {key: maps[key].astype(np.float32) for key in ('continuum', 'coefficients', 'rms')}
    out['count'] = maps['count']
    # what is stored unchanged keeps its bits, NaN payloads included: the non-finite samples of a
    # fitted element, and every channel that is not filled
    filled = np.asarray(filled) != 0
    keep = np.broadcast_to(~filled.reshape((-1,) + (1,) * (cube.ndim - 1)), cube.shape) \
        | (maps['fitted'][np.newaxis] & ~np.isfinite(cube))
    rounded = np.where(keep, cube, rounded)
    return rounded, out


class ImContSub(CubeOperator):
    """``kimg_imcontsub`` for cubes of shape ``cube_shape`` = (C, P, H, W).  ``op(cube)`` takes a
    :class:`cube.SpectralCube` and works in place; ``op(cube, out=other)`` writes the line cube into
    another SpectralCube of the same shape and frequencies and leaves the source alone -- ``other``'s
    ``filled`` and ``noise`` take the source's.  Returns ``{name: MapArray [P][H][W]}`` for
    ``outputs``, a subset of 'continuum', 'rms' (float32), 'count' (int32) and 'coefficients'
    (float32 [K][P][H][W]); maps that were not asked for are not allocated.  The call is asynchronous
    on ``command_queue`` once the per-channel tables (8 (K + 1) bytes a channel) are on the device.

    ``op(array, filled=..., frequencies=..., noise=..., out=array2)`` takes plain
    :class:`accel.DeviceArray` [C][P][H][W] instead, whose [P][H][W] plane is dense while the channel
    axis may have any pitch (a view of a larger tensor), each array its own.  ``out`` must be the
    array itself (or None: in place) or share no memory with it."""

    def __init__(self, template, command_queue, cube_shape, outputs=DEFAULT_OUTPUTS):
        super().__init__(template, command_queue, cube_shape)
        self.params.mask(self.cube_shape[0])
        try:
            outputs = tuple(outputs)
        except TypeError:
            raise ValueError('outputs must be a sequence of map names') from None
        if not outputs or len(set(outputs)) != len(outputs) \
                or any(name not in OUTPUT_BITS for name in outputs):
            raise ValueError('outputs must be distinct names from {}'.format(sorted(OUTPUT_BITS)))
        self.outputs = outputs
        self._tables = None

    def __call__(self, cube, filled=None, frequencies=None, noise=None, out=None):
        params = self.params
        C = self.cube_shape[0]
        K = params.order + 1
        array = self._array(cube, 'cube')
        filled = self._own_filled(cube, filled, frequencies=frequencies, noise=noise)
        if isinstance(cube, SpectralCube):
            frequencies, noise = cube.frequencies, cube.noise
        check_out_cube(cube, out, 'line cube')
        target = array if out is None else self._array(out, 'out')
        filled, fit, w, B, bref, min_samples = params.tables(C, filled, frequencies, noise)
        pitch = channel_pitch(array)
        target_pitch = channel_pitch(target)
        queue = self.command_queue
        context = queue.context
        # one upload: w, then the basis
        tables = np.concatenate((w, B.reshape(-1)))
        if self._tables is None or self._tables.shape != tables.shape:
            self._tables = accel.DeviceArray(context, tables.shape, np.float64, queue=queue)
        self._tables.set(queue, tables)
        plane = self.cube_shape[1:]
        M = int(np.prod(plane))
        maps = {}
        for name in self.outputs:
            shape = (K,) + plane if name == 'coefficients' else plane
            maps[name] = MapArray(context, shape, np.int32 if name == 'count' else np.float32,
                                  queue=queue)
        bits = 0
        for name in maps:
            bits |= OUTPUT_BITS[name]
        array.used_on(queue)
        target.used_on(queue)
        pointer = {name: maps[name].ptr if name in maps else None for name in OUTPUT_BITS}
        reference = [float(x) for x in bref] + [0.0] * (4 - K)
        check(lib().kimg_imcontsub(
            array.ptr, pitch, target.ptr, target_pitch, C, M,
            filled.ctypes.data_as(ctypes.c_void_p), fit.ctypes.data_as(ctypes.c_void_p),
            w.ctypes.data_as(ctypes.c_void_p), self._tables.ptr, self._tables.ptr + 8 * C,
            params.order, *reference, min_samples, bits, pointer['continuum'],
            pointer['coefficients'], M, pointer['rms'], pointer['count'], queue.handle),
            'kimg_imcontsub')
        mark_ready(queue, maps.values())
        carry_over(cube, out)
        return maps


class ImContSubTemplate(OperatorTemplate):
    params_type = ImContSubParameters
    operator = ImContSub
