"""Imaging (density) weights: natural, uniform and robust.

Operator surface of the reference's ``katsdpimager.weight`` (GridWeights,
DensityWeights, MeanWeight, compound Weights; weight.py:55-538) on libkimg.so.
See the reference module docstring (weight.py:3-44) for the definitions [Bri95].
"""
import ctypes
import enum
import math
import sys

import numpy as np

from . import accel
from ._lib import lib, check, UVTaper
from .image_plane import ImageTemplate, check_polarizations, plane_args


class WeightType(enum.Enum):
    """weight.py:55-58."""
    NATURAL = 0
    UNIFORM = 1
    ROBUST = 2


def _non_negative(name, value):
    value = float(value)
    if not math.isfinite(value) or value < 0:
        raise ValueError('{} must be finite and not negative, not {!r}'.format(name, value))
    return value


class UVTaperParameters:
    """A uv taper and uv range on top of the density weights (CASA ``uvtaper`` / ``uvrange``,
    WSClean ``-taper-gaussian``, ``-minuv-l``, ``-maxuv-l``, ``-taper-inner-tukey``,
    ``-taper-edge-tukey``): every cell of the weights grid is multiplied by T = G * inner * outer.

    ``gaussian``: the image-plane FWHM of the beam the taper alone would produce, one float
    (circular) or ``(major, minor, position_angle)``, in the l/m units of :mod:`parameters` (radians
    for small angles).  ``position_angle`` is in radians and is the angle :func:`beam.fit_beam`
    reports as ``Beam.theta``: the major axis stands at that angle from axis 0 of the image (rows,
    m) towards axis 1 (columns, l), in [0, pi).  With u_maj = v cos(pa) + u sin(pa) and
    u_min = -v sin(pa) + u cos(pa) (wavelengths),
    G = exp(-(pi^2 / (4 ln 2)) (major^2 u_maj^2 + minor^2 u_min^2)).

    ``min_uv``, ``max_uv`` (wavelengths) cut on r = hypot(u, v): T = 0 for r < min_uv and for
    r > max_uv.  ``inner_tukey`` / ``outer_tukey`` (wavelengths) put a raised-cosine ramp
    0.5 (1 - cos(pi x)) over [min_uv, min_uv + inner_tukey] and its mirror image over
    [max_uv - outer_tukey, max_uv].  :func:`uv_taper_host` is the numpy statement of all this."""

    def __init__(self, gaussian=None, min_uv=None, max_uv=None, inner_tukey=0.0, outer_tukey=0.0):
        if gaussian is None:
            self.gaussian = None
        else:
            if np.ndim(gaussian) == 0:
                gaussian = (gaussian, gaussian, 0.0)
            if len(gaussian) != 3:
                raise ValueError('gaussian is one FWHM or (major, minor, position_angle)')
            major = _non_negative('gaussian major', gaussian[0])
            minor = _non_negative('gaussian minor', gaussian[1])
            angle = float(gaussian[2])
            if not math.isfinite(angle):
                raise ValueError('gaussian position_angle must be finite')
            if minor > major:
                raise ValueError('gaussian minor {!r} exceeds major {!r}'.format(minor, major))
            self.gaussian = (major, minor, angle)
        self.min_uv = None if min_uv is None else _non_negative('min_uv', min_uv)
        self.max_uv = None if max_uv is None else _non_negative('max_uv', max_uv)
        self.inner_tukey = _non_negative('inner_tukey', inner_tukey)
        self.outer_tukey = _non_negative('outer_tukey', outer_tukey)
        low = self.min_uv or 0.0
        if self.max_uv is not None:
            if low >= self.max_uv:
                raise ValueError('min_uv {!r} is not below max_uv {!r}'.format(low, self.max_uv))
            if low + self.inner_tukey > self.max_uv - self.outer_tukey:
                raise ValueError('the inner and outer ramps overlap')
        elif self.outer_tukey > 0:
            raise ValueError('outer_tukey needs max_uv')

    @classmethod
    def from_arcsec(cls, gaussian=None, position_angle_deg=0.0, **kwargs):
        """``gaussian`` in arcseconds -- one FWHM or ``(major, minor)`` -- and the position angle
        in degrees; everything else as the constructor takes it."""
        if gaussian is not None:
            scale = math.pi / (180.0 * 3600.0)
            if np.ndim(gaussian) == 0:
                gaussian = (gaussian, gaussian)
            major, minor = gaussian
            gaussian = (float(major) * scale, float(minor) * scale, math.radians(position_angle_deg))
        return cls(gaussian, **kwargs)

    def _key(self):
        return (self.gaussian, self.min_uv, self.max_uv, self.inner_tukey, self.outer_tukey)

    def __eq__(self, other):
        return isinstance(other, UVTaperParameters) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return ('UVTaperParameters(gaussian={!r}, min_uv={!r}, max_uv={!r}, inner_tukey={!r}, '
                'outer_tukey={!r})').format(*self._key())

    def coefficients(self):
        """The seven doubles of ``kimg_uv_taper`` (include/kimg.h): the Gaussian's quadratic form
        (u u, u v, v v), the cut radii -- no cut is 0 and the largest double -- and the ramps."""
        quad = (0.0, 0.0, 0.0)
        if self.gaussian is not None:
            major, minor, angle = self.gaussian
            k = math.pi ** 2 / (4.0 * math.log(2.0))
            c, s = math.cos(angle), math.sin(angle)
            quad = (k * (major * major * s * s + minor * minor * c * c),
                    2.0 * k * (major * major - minor * minor) * s * c,
                    k * (major * major * c * c + minor * minor * s * s))
        return quad + (self.min_uv or 0.0, sys.float_info.max if self.max_uv is None else self.max_uv,
                       self.inner_tukey, self.outer_tukey)


def uv_taper_host(shape, image_size, params):
    """T of :class:`UVTaperParameters` on a weights grid: float64 [H][W] for ``shape`` = (..., H, W),
    cell (x, y) standing at u = (x - W/2) / image_size, v = (y - H/2) / image_size wavelengths
    (``image_size``: ``parameters.ImageParameters.image_size``).  The steps of
    kimg_density_weights_taper (include/kimg.h) in numpy float64, in its order."""
    H, W = int(shape[-2]), int(shape[-1])
    quad_uu, quad_uv, quad_vv, min_uv, max_uv, inner, outer = params.coefficients()
    step = 1.0 / float(image_size)
    u = ((np.arange(W) - W // 2).astype(np.float64) * step)[np.newaxis, :]
    v = ((np.arange(H) - H // 2).astype(np.float64) * step)[:, np.newaxis]
    t = np.exp(-((quad_uu * u * u + quad_uv * u * v) + quad_vv * v * v))
    r = np.sqrt(u * u + v * v)
    if inner > 0:
        ramp = np.sin((0.5 * np.pi) * ((r - min_uv) / inner)) ** 2
        t = np.where(r < min_uv + inner, t * ramp, t)
    if outer > 0:
        ramp = np.sin((0.5 * np.pi) * ((max_uv - r) / outer)) ** 2
        t = np.where(r > max_uv - outer, t * ramp, t)
    return np.where((r < min_uv) | (r > max_uv), 0.0, t)


class _WeightsStepTemplate(ImageTemplate):
    """The weights grid is float32 whatever the image is: no dtype."""
    def __init__(self, context, num_polarizations, tuning=None):
        lib()
        self.context = context
        self.num_polarizations = num_polarizations


class GridWeights(accel.Operation):
    """Accumulate statistical weights on the grid without convolution (weight.py:90-183).
    Slots: **uv** int16 [max_vis][4], **weights** float32 [max_vis][pols],
    **grid** float32 [pols][H][W]."""

    def __init__(self, template, command_queue, grid_shape, max_vis, allocator=None):
        super().__init__(command_queue, allocator)
        self.template = template
        check_polarizations(template, grid_shape)
        if grid_shape[1] % 2 or grid_shape[2] % 2:
            raise ValueError('Odd-sized grid not currently supported')
        self.max_vis = max_vis
        self.slots['grid'] = accel.IOSlot(grid_shape, np.float32)
        self.slots['uv'] = accel.IOSlot((max_vis, accel.Dimension(4, exact=True)), np.int16)
        self.slots['weights'] = accel.IOSlot(
            (max_vis, accel.Dimension(template.num_polarizations, exact=True)), np.float32)
        self._num_vis = 0

    @property
    def num_vis(self):
        return self._num_vis

    @num_vis.setter
    def num_vis(self, n):
        if n < 0 or n > self.max_vis:
            raise ValueError('Number of visibilities {} is out of range 0..{}'.format(
                n, self.max_vis))
        self._num_vis = n

    def _run(self):
        rc = lib().kimg_grid_weights(*plane_args(self.buffer('grid')), self.buffer('uv').ptr,
                                     self.buffer('weights').ptr, self._num_vis,
                                     self.command_queue.handle)
        check(rc, 'kimg_grid_weights')


class GridWeightsTemplate(_WeightsStepTemplate):
    """weight.py:61-87."""
    operator = GridWeights


class DensityWeights(accel.Operation):
    """In place W -> 1/(a W + b) (0 where W == 0); returns (rms, normalized_rms)
    (weight.py:217-293).  Slot **sums** is float64 [3] here.

    ``taper`` (:class:`UVTaperParameters`, with the ``image_size`` of the image the grid belongs
    to) multiplies every cell by the taper in the same pass (kimg_density_weights_taper); the sums,
    and so the two figures returned, are those of the tapered weights."""

    def __init__(self, template, command_queue, grid_shape, allocator=None, taper=None,
                 image_size=None):
        super().__init__(command_queue, allocator)
        self.template = template
        check_polarizations(template, grid_shape)
        self.a = 1.0
        self.b = 0.0
        self.taper = taper
        self.image_size = None
        self._taper_struct = None
        if taper is not None:
            if image_size is None or not math.isfinite(image_size) or image_size <= 0:
                raise ValueError('a taper needs the image_size of the grid')
            if grid_shape[1] % 2 or grid_shape[2] % 2:
                raise ValueError('Odd-sized grid not currently supported')
            self.image_size = float(image_size)
            self._taper_struct = UVTaper(*taper.coefficients())
        self.slots['grid'] = accel.IOSlot(grid_shape, np.float32)
        self.slots['sums'] = accel.IOSlot((3,), np.float64)

    def _run(self, mean_sums=None, robust=None):
        """``mean_sums`` (device float64 [2] as :class:`MeanWeight` leaves it) and ``robust``: a =
        robust / (mean weight) worked out on the device instead of ``self.a``."""
        sums = self.buffer('sums')
        grid = plane_args(self.buffer('grid'))
        if self._taper_struct is not None:
            step = 1.0 / self.image_size
            rc = lib().kimg_density_weights_taper(
                sums.ptr, *grid, self.a, self.b,
                mean_sums.ptr if mean_sums is not None else None,
                float(robust) if mean_sums is not None else 0.0, step, step,
                ctypes.byref(self._taper_struct), self.command_queue.handle)
            check(rc, 'kimg_density_weights_taper')
        elif mean_sums is not None:
            rc = lib().kimg_density_weights_robust(sums.ptr, *grid, mean_sums.ptr, float(robust),
                                                   self.b, self.command_queue.handle)
            check(rc, 'kimg_density_weights_robust')
        else:
            rc = lib().kimg_density_weights(sums.ptr, *grid, self.a, self.b,
                                            self.command_queue.handle)
            check(rc, 'kimg_density_weights')
        s = sums.get(self.command_queue)
        if self._taper_struct is not None and not s[1] > 0:
            raise ValueError('the uv taper cuts every cell that holds a visibility: {!r}'.format(
                self.taper))
        rms = np.sqrt(s[2]) / s[1]
        return rms, rms * np.sqrt(s[0])


class DensityWeightsTemplate(_WeightsStepTemplate):
    """weight.py:186-214."""
    operator = DensityWeights


class MeanWeight(accel.Operation):
    """sum W^2 / sum W over the first polarization (weight.py:326-376)."""

    def __init__(self, template, command_queue, grid_shape, allocator=None):
        super().__init__(command_queue, allocator)
        self.template = template
        self.slots['grid'] = accel.IOSlot(grid_shape, np.float32)
        self.slots['sums'] = accel.IOSlot((2,), np.float64)

    def _run(self):
        s = self.enqueue().get(self.command_queue)
        return s[1] / s[0]

    def enqueue(self):
        """The two sums, left on the device (returns the buffer)."""
        grid = self.buffer('grid')
        sums = self.buffer('sums')
        P, H, W = grid.shape
        rc = lib().kimg_mean_weight(sums.ptr, grid.ptr, W, W, H, self.command_queue.handle)
        check(rc, 'kimg_mean_weight')
        return sums


class MeanWeightTemplate(ImageTemplate):
    """weight.py:296-324.  Only the context: the first polarization of a float32 grid."""
    operator = MeanWeight

    def __init__(self, context, tuning=None):
        lib()
        self.context = context


class WeightsTemplate:
    """weight.py:379-416.  ``taper`` (:class:`UVTaperParameters` or None): with one, natural
    weighting too accumulates the weights on the grid and runs the density pass (a = 0, b = 1), so
    that only cells that received a visibility carry the taper and ``finalize()`` has real sums."""
    def __init__(self, context, weight_type, num_polarizations,
                 grid_weights_tuning=None, mean_weight_tuning=None, density_weights_tuning=None,
                 taper=None):
        lib()
        self.context = context
        self.weight_type = weight_type
        self.num_polarizations = num_polarizations
        self.taper = taper
        natural = weight_type == WeightType.NATURAL and taper is None
        self.grid_weights = None if natural else GridWeightsTemplate(context, num_polarizations)
        self.density_weights = None if natural else DensityWeightsTemplate(context,
                                                                           num_polarizations)
        self.mean_weight = MeanWeightTemplate(context) if weight_type == WeightType.ROBUST \
            else None

    def instantiate(self, *args, **kwargs):
        return Weights(self, *args, **kwargs)


class Weights(accel.OperationSequence):
    """Compound imaging-weights operation (weight.py:419-538): ``clear()``, ``grid(N)``
    per batch, then ``finalize()`` -> (rms, normalized_rms).  Slots **grid** (and **uv**,
    **weights** unless natural weighting without a taper).  The template's taper needs
    ``image_size`` (``parameters.ImageParameters.image_size`` of the image the grid belongs to)."""

    def __init__(self, template, command_queue, grid_shape, max_vis, allocator=None,
                 image_size=None):
        self.template = template
        self.taper = template.taper
        self.image_size = image_size
        operations = []
        compounds = {'grid': []}
        self._grid_weights = self._mean_weight = self._density_weights = None
        self.robustness = None
        if template.grid_weights is not None:
            self._grid_weights = template.grid_weights.instantiate(
                command_queue, grid_shape, max_vis, allocator)
            operations.append(('grid_weights', self._grid_weights))
            compounds['grid'].append('grid_weights:grid')
            compounds['uv'] = ['grid_weights:uv']
            compounds['weights'] = ['grid_weights:weights']
        if template.mean_weight is not None:
            self._mean_weight = template.mean_weight.instantiate(
                command_queue, grid_shape, allocator)
            operations.append(('mean_weight', self._mean_weight))
            compounds['grid'].append('mean_weight:grid')
            self.robustness = 0.0
        if template.density_weights is not None:
            self._density_weights = template.density_weights.instantiate(
                command_queue, grid_shape, allocator, template.taper, image_size)
            if template.weight_type == WeightType.NATURAL:
                self._density_weights.a, self._density_weights.b = 0.0, 1.0
            operations.append(('density_weights', self._density_weights))
            compounds['grid'].append('density_weights:grid')
        super().__init__(command_queue, operations, compounds, allocator=allocator)
        if not compounds['grid']:
            # natural weighting: just a grid that finalize() fills with ones
            self.slots['grid'] = accel.IOSlot(grid_shape, np.float32)

    def _run(self):
        raise NotImplementedError('Weights should not be used as a callable')

    def clear(self):
        self.ensure_all_bound()
        if self._grid_weights is not None:
            self.buffer('grid').zero(self.command_queue)

    def grid(self, N):
        self.ensure_all_bound()
        if self._grid_weights is not None:
            self._grid_weights.num_vis = N
            return self._grid_weights()

    def finalize(self):
        self.ensure_all_bound()
        if self._mean_weight is not None:
            # weight.py:525-531 without the host between the two kernels: S2 = robust / mean weight
            # is worked out where the sums are (kimg_density_weights_robust)
            self._density_weights.b = 1.0
            return self._density_weights._run(self._mean_weight.enqueue(),
                                              (5 * 10**(-self.robustness))**2)
        if self._density_weights is not None:
            return self._density_weights()
        grid = self.buffer('grid')
        check(lib().kimg_fill(grid.ptr, int(np.prod(grid.shape)), 1.0,
                              self.command_queue.handle), 'kimg_fill')
        return None, 1.0
