"""Primary-beam models and correction.

The reference ends every channel by sampling a radially symmetric beam model on the pixel grid,
dividing the model and the residual image by the beam power and blanking what lies below a cutoff
(frontend.py:587-608, primary_beam.py).  Here the model's row for the channel's frequency goes to
the device (a few hundred floats) and one pass of ``kimg_primary_beam`` (include/kimg.h) samples
the beam and corrects both images.

The host side is numpy only: :class:`RadialBeam` (the contract of the reference's
``TrivialPrimaryBeam``), :func:`sample_host` and :func:`correct_host` -- the numpy statement of
the device contract, which the device meets bit for bit -- and :func:`sample_float64`, the
reference's ``_sample_impl`` restated in float64, against which tests bound what the float32
contract costs.
"""
import numpy as np

from . import accel
from ._lib import lib, check, PRIMARY_BEAM_MAX_SAMPLES
from .image_plane import ImageTemplate, check_image_shape, plane2d_args

SPEED_OF_LIGHT = 299792458.0        # m / s


def _cosine_taper_voltage(r):
    """cos(pi r) / (1 - 4 r^2) for r >= 0, written as (pi / 4) sinc(r - 1/2) / (r + 1/2)
    (cos(pi r) = -sin(pi (r - 1/2)), 1 - 4 r^2 = -4 (r - 1/2) (r + 1/2)): no cancellation near the
    removable singularity at r = 1/2, where it is pi / 4."""
    r = np.asarray(r, np.float64)
    return (np.pi / 4.0) * np.sinc(r - 0.5) / (r + 0.5)


def _cosine_taper_half_power():
    """The r at which the cosine-tapered aperture's power is 1/2, by bisection: the voltage falls
    from pi / 4 at r = 1/2 to 1/3 at r = 1."""
    target = np.sqrt(0.5)
    lo, hi = 0.5, 1.0
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        if _cosine_taper_voltage(mid) > target:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


class RadialBeam:
    """A radially symmetric, antenna-, elevation- and polarization-independent, real-valued beam
    (the reference's ``TrivialPrimaryBeam``, primary_beam.py:56-172).

    ``samples[f][i]`` is the voltage pattern at radius ``i * step`` (sine projection) for
    ``frequencies[f]`` (Hz, increasing); at least 2 radial samples.  ``band`` names the receiver
    band (free text)."""

    def __init__(self, step, frequencies, samples, band=None):
        self.step = float(step)
        self.frequencies = np.array(frequencies, np.float64, ndmin=1)
        self.samples = np.array(samples)
        self.band = band
        if not np.isfinite(self.step) or self.step <= 0:
            raise ValueError('step must be finite and above 0, not {!r}'.format(step))
        if self.samples.ndim != 2:
            raise ValueError('samples must be 2-D (frequency, radius)')
        if self.frequencies.ndim != 1 or len(self.samples) != len(self.frequencies):
            raise ValueError('frequency and samples have inconsistent shape')
        if self.samples.shape[1] < 2:
            raise ValueError('samples needs at least 2 radial samples')
        if len(self.frequencies) == 0 or np.any(np.diff(self.frequencies) <= 0):
            raise ValueError('frequencies must be increasing')

    def inradius(self, frequency=None):
        """The radius of the last sample: beyond it the beam is NaN."""
        return self.step * (self.samples.shape[1] - 1)

    def frequency_range(self):
        return float(self.frequencies[0]), float(self.frequencies[-1])

    def row(self, frequency):
        """The voltage pattern at ``frequency`` (Hz), float32 [R]: linear in frequency between the
        bracketing rows, ``a (1 - t) + b t`` in float64, rounded once.  All NaN outside the
        frequency range (the reference returns NaN there and raises nothing)."""
        frequency = float(frequency)
        f = self.frequencies
        R = self.samples.shape[1]
        if not f[0] <= frequency <= f[-1]:      # (a NaN frequency too)
            return np.full(R, np.nan, np.float32)
        hi = int(np.searchsorted(f, frequency, side='left'))
        if f[hi] == frequency:
            return self.samples[hi].astype(np.float32)
        lo = hi - 1
        t = (frequency - f[lo]) / (f[hi] - f[lo])
        a = self.samples[lo].astype(np.float64)
        b = self.samples[hi].astype(np.float64)
        return (a * (1.0 - t) + b * t).astype(np.float32)

    def save(self, filename):
        """Write the model as ``.npz`` (numpy appends the suffix to a name without it)."""
        np.savez(filename, step=np.float64(self.step), frequencies=self.frequencies,
                 samples=self.samples, band=np.array('' if self.band is None else str(self.band)))

    @classmethod
    def load(cls, filename):
        with np.load(filename) as data:
            band = str(data['band'])
            return cls(float(data['step']), data['frequencies'], data['samples'], band or None)

    @classmethod
    def cosine_taper(cls, fwhm, frequency_ref, frequencies, step, radius, band=None):
        """The beam of a cosine-tapered aperture, V(r) = cos(pi r) / (1 - 4 r^2) with
        r = c rho / fwhm(nu) and fwhm(nu) = fwhm * frequency_ref / nu: full width at half maximum
        (of the power) ``fwhm`` at ``frequency_ref``, in l/m units, narrowing as 1 / nu.  c makes
        V^2 = 1/2 at rho = fwhm / 2.  Tabulated at ``frequencies`` (Hz, increasing) every ``step``
        out to at least ``radius``."""
        frequencies = np.array(frequencies, np.float64, ndmin=1)
        c = 2.0 * _cosine_taper_half_power()
        count = max(2, int(np.ceil(float(radius) / float(step) - 1e-9)) + 1)
        rho = np.arange(count, dtype=np.float64) * float(step)
        widths = float(fwhm) * float(frequency_ref) / frequencies
        samples = _cosine_taper_voltage(c * rho[np.newaxis, :] / widths[:, np.newaxis])
        return cls(step, frequencies, samples, band)

    def _key(self):
        return (self.step, self.frequencies.tobytes(), self.samples.shape, str(self.samples.dtype),
                self.samples.tobytes(), self.band)

    def __eq__(self, other):
        return isinstance(other, RadialBeam) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return 'RadialBeam(step={!r}, {} frequencies {!r}..{!r} Hz, {} samples, band={!r})'.format(
            self.step, len(self.frequencies), float(self.frequencies[0]),
            float(self.frequencies[-1]), self.samples.shape[1], self.band)


class PrimaryBeamParameters:
    """What a channel's primary-beam correction needs: the ``model`` (:class:`RadialBeam`) and the
    ``cutoff``, the beam power below which the images are blanked (the reference's
    ``--primary-beam-cutoff``, default 0.1)."""

    def __init__(self, model, cutoff=0.1):
        if not callable(getattr(model, 'row', None)) or not hasattr(model, 'step'):
            raise TypeError('model must be a RadialBeam')
        cutoff = float(cutoff)
        if not np.isfinite(cutoff):
            raise ValueError('cutoff must be finite, not {!r}'.format(cutoff))
        self.model = model
        self.cutoff = cutoff

    def _key(self):
        return (self.model, self.cutoff)

    def __eq__(self, other):
        return isinstance(other, PrimaryBeamParameters) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return 'PrimaryBeamParameters(model={!r}, cutoff={!r})'.format(*self._key())


def inv_step32(step):
    """The float32 the device multiplies by: the nearest to 1 / step, formed on the host."""
    return np.float32(1.0 / float(step))


def sample_host(row, step, width, height, lm_scale, lm_bias):
    """The beam power on the pixel grid, float32 [height][width]: the contract of
    ``kimg_primary_beam`` (include/kimg.h) in numpy float32, one rounding per line.  ``row``:
    float32 [R]; ``lm_scale`` = pixel_size and ``lm_bias`` = -pixels / 2 * pixel_size as
    :class:`imaging.Imaging` forms them."""
    row = np.asarray(row, np.float32)
    R = len(row)
    scale, bias = np.float32(lm_scale), np.float32(lm_bias)
    inv_step = inv_step32(step)
    with np.errstate(invalid='ignore', over='ignore'):
        l = np.arange(width, dtype=np.float32) * scale
        l = l + bias
        m = np.arange(height, dtype=np.float32) * scale
        m = m + bias
        ll = (l * l)[np.newaxis, :]
        mm = (m * m)[:, np.newaxis]
        s = np.sqrt(ll + mm)
        s = s * inv_step
        inside = s < np.float32(R - 1)          # pos < R - 1; false for a NaN
        pos = np.where(inside, s, np.float32(0)).astype(np.int32)
        frac = s - pos.astype(np.float32)
        delta = row[pos + 1] - row[pos]
        delta = delta * frac
        v = row[pos] + delta
        power = v * v
    assert power.dtype == np.float32
    return np.where(inside, power, np.float32(np.nan))


def sample_float64(row, step, width, height, lm_scale, lm_bias):
    """The reference's ``_sample_impl`` (primary_beam.py:22-53) on the pixel grid in float64:
    radius / step, truncated; float64 [height][width].  For tests: what the float32 contract of
    :func:`sample_host` costs."""
    row = np.asarray(row, np.float64)
    deltas = row[1:] - row[:-1]
    l = (np.arange(width, dtype=np.float64) * float(lm_scale) + float(lm_bias))[np.newaxis, :]
    m = (np.arange(height, dtype=np.float64) * float(lm_scale) + float(lm_bias))[:, np.newaxis]
    radius_steps = np.sqrt(l * l + m * m) / float(step)
    inside = radius_steps < len(deltas)
    pos = np.where(inside, radius_steps, 0.0).astype(np.int64)
    value = row[pos] + deltas[pos] * (radius_steps - pos)
    return np.where(inside, value * value, np.nan)


def correct_host(power, model, dirty, threshold):
    """The correction of ``kimg_primary_beam`` on host arrays, in place: where
    ``power >= threshold`` model and dirty are divided by the power, elsewhere -- a NaN power
    included -- the model becomes 0 and the dirty image NaN.  ``power``: float32 [H][W];
    ``model``, ``dirty``: float32 [P][H][W].  Returns ``keep``."""
    power = np.asarray(power, np.float32)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        keep = power >= np.float32(threshold)
        for image, blank in ((model, np.float32(0)), (dirty, np.float32(np.nan))):
            assert image.dtype == np.float32
            image[...] = np.where(keep, image / power, blank)
    return keep


class PrimaryBeam(accel.Operation):
    """Sample the beam model's row on the pixel grid and correct model and dirty by its power
    (``kimg_primary_beam``).  Slots: **beam_power** [H][W], **model** and **dirty** [P][H][W].
    ``row`` is the device copy of the model's row (:meth:`set_model_row`), ``step`` its radial
    step, ``lm_scale`` / ``lm_bias`` the pixel grid (l = x * lm_scale + lm_bias), ``threshold``
    the beam power below which the images are blanked."""

    def __init__(self, template, command_queue, image_shape, allocator=None):
        super().__init__(command_queue, allocator)
        check_image_shape(template, image_shape)
        self.template = template
        self.slots['beam_power'] = accel.IOSlot(image_shape[1:], template.dtype)
        self.slots['model'] = accel.IOSlot(image_shape, template.dtype)
        self.slots['dirty'] = accel.IOSlot(image_shape, template.dtype)
        self.row = None
        self.step = None
        self.lm_scale = 0.0
        self.lm_bias = 0.0
        self.threshold = 0.0

    def set_model_row(self, row, step):
        """Upload ``row`` (float32 [R], ``RadialBeam.row``) whose samples are ``step`` apart."""
        row = np.ascontiguousarray(row, np.float32)
        if row.ndim != 1 or not 2 <= len(row) <= PRIMARY_BEAM_MAX_SAMPLES:
            raise ValueError('a row has 2 to {} samples, not shape {}'.format(
                PRIMARY_BEAM_MAX_SAMPLES, row.shape))
        if not float(step) > 0:
            raise ValueError('step must be above 0, not {!r}'.format(step))
        if self.row is None or self.row.shape != row.shape:
            self.row = accel.DeviceArray(self.command_queue.context, row.shape, np.float32,
                                         queue=self.command_queue)
        self.row.set(self.command_queue, row)
        self.step = float(step)

    def _launch(self, images):
        if self.row is None:
            raise RuntimeError('set_model_row has not been called')
        beam = self.buffer('beam_power')
        H, W = beam.shape
        model = self.buffer('model').ptr if images else None
        dirty = self.buffer('dirty').ptr if images else None
        rc = lib().kimg_primary_beam(
            *plane2d_args(beam), model, dirty, W, H * W, W, H, self.template.num_polarizations,
            self.row.ptr, self.row.shape[0], float(inv_step32(self.step)), self.lm_scale,
            self.lm_bias, self.threshold, self.command_queue.handle)
        check(rc, 'kimg_primary_beam')

    def _run(self):
        self._launch(True)

    def sample(self):
        """Fill **beam_power** only; the images are not touched (and need not be bound)."""
        self.ensure_bound('beam_power')
        self._launch(False)


class PrimaryBeamTemplate(ImageTemplate):
    """float32 only."""
    operator = PrimaryBeam

    def __init__(self, context, dtype, num_polarizations, tuning=None):
        super().__init__(context, dtype, num_polarizations, tuning)
        if not 1 <= num_polarizations <= 4:
            raise ValueError('1 to 4 polarizations, not {}'.format(num_polarizations))
