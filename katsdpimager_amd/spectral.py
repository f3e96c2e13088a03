"""Spectral smoothing and channel averaging of raw visibilities: a short non-negative FIR along the
channel axis followed by an integer decimation, weighted and aware of flags (CASA's ``hanningsmooth``
and ``mstransform(chanaverage=True, chanbin=n)`` / ``split(width=n)``, MIRIAD's ``hanning``), ahead of
the continuum fit and of preprocessing.

The reference images the channels it is given; this is the operator a spectral-line user runs
first.  The contract is written in include/kimg.h ("Spectral filter"); :func:`filter_host` is the
same contract as numpy, and the executable specification the device (csrc/spectral.hip,
:class:`SpectralFilter`) is tested against.
``loader.preprocess_visibilities(..., spectral=SpectralParameters.hanning())`` puts the operator
between the loader and the collector.
"""
import ctypes

import numpy as np

from . import accel
from ._lib import lib, check
from .channel_block import ChannelOperator, OperatorTemplate, channel_pitch, check_block

#: KIMG_SPECTRAL_MAX_TAPS
MAX_TAPS = 9
#: KIMG_SPECTRAL_MAX_BIN
MAX_BIN = 64


class SpectralParameters:
    """``taps``: the smoothing filter, an odd number (at most 9) of finite values >= 0 whose middle
    one is above 0 and sits on the output channel.  ``bin``: n channels are then averaged into one,
    1 to 64.  ``min_coverage`` in (0, 1]: an output sample is kept when the coefficients of its
    usable inputs add up to at least this fraction of all its coefficients.  The filter normalises
    itself sample by sample (flagged inputs drop out), so the scale of ``taps`` does not matter."""

    def __init__(self, taps=(1.0,), bin=1, min_coverage=0.5):
        try:
            taps = np.array(taps, np.float64, ndmin=1)
        except (TypeError, ValueError):
            raise ValueError('taps must be numbers') from None
        if taps.ndim != 1 or len(taps) % 2 != 1 or len(taps) > MAX_TAPS:
            raise ValueError('taps must be an odd number of values, at most {}'.format(MAX_TAPS))
        if not np.all(np.isfinite(taps)) or np.any(taps < 0):
            raise ValueError('taps must be finite and not negative')
        if not taps[len(taps) // 2] > 0:
            raise ValueError('the centre tap must be above 0')
        try:
            as_int = int(bin)
        except (TypeError, ValueError):
            raise ValueError('bin must be an integer') from None
        if as_int != bin or not 1 <= as_int <= MAX_BIN:
            raise ValueError('bin must be an integer from 1 to {}'.format(MAX_BIN))
        min_coverage = float(min_coverage)
        if not 0.0 < min_coverage <= 1.0:           # (false for NaN)
            raise ValueError('min_coverage must lie in (0, 1]')
        self.taps = taps
        self.taps.setflags(write=False)
        self.bin = as_int
        self.min_coverage = min_coverage

    @classmethod
    def hanning(cls, bin=1, min_coverage=0.5):
        """Hanning smoothing (1/4, 1/2, 1/4), then ``bin`` channels to one."""
        return cls((0.25, 0.5, 0.25), bin, min_coverage)

    @classmethod
    def average(cls, n, min_coverage=0.5):
        """``n`` channels to one, no smoothing."""
        return cls((1.0,), n, min_coverage)

    def coefficients(self):
        """(g, offset, step): the combined filter ``taps (*) ones(bin)`` in float64, the index in it
        of the first channel of the bin, and the decimation.  Output o reads the inputs
        ``o * step - offset + i`` for i over g."""
        g = np.convolve(self.taps, np.ones(self.bin, np.float64))
        return g, len(self.taps) // 2, self.bin

    def min_sum(self):
        """The coverage an output sample needs, on the scale of the coefficients."""
        return self.min_coverage * float(self.coefficients()[0].sum())

    def output_channels(self, num_channels_in):
        """``C_in // bin``; the ``C_in % bin`` channels left over enter only through the smoothing."""
        num_channels_in = int(num_channels_in)
        if num_channels_in < self.bin:
            raise ValueError('{} channels cannot be averaged {} to one'.format(num_channels_in, self.bin))
        return num_channels_in // self.bin

    def output_frequencies(self, frequencies):
        """float64 [C_out]: the mean of the input frequencies of every bin."""
        frequencies = np.asarray(frequencies, np.float64)
        if frequencies.ndim != 1:
            raise ValueError('frequencies must have one entry per channel')
        C_out = self.output_channels(len(frequencies))
        return frequencies[:C_out * self.bin].reshape(C_out, self.bin).mean(axis=1)

    def __repr__(self):
        return 'SpectralParameters(taps={!r}, bin={}, min_coverage={})'.format(
            tuple(self.taps.tolist()), self.bin, self.min_coverage)


def filter_host_double(vis, weights, params):
    """The contract up to its last step: (vis complex128 BEFORE the one rounding to complex64,
    weights float64 before theirs to float32, kept bool), all [C_out][N][Q].  Where ``kept`` is
    False both are 0."""
    vis = np.asarray(vis)
    weights = np.asarray(weights)
    check_block(vis, weights)
    C_in = vis.shape[0]
    g, offset, step = params.coefficients()
    min_sum = params.min_sum()
    C_out = params.output_channels(C_in)
    usable = (weights > 0) & np.isfinite(vis.real) & np.isfinite(vis.imag)
    w = np.where(usable, weights.astype(np.float64), 0.0)
    # (w * v is exact: two 24-bit significands)
    with np.errstate(invalid='ignore'):
        wr = np.where(usable, w * vis.real.astype(np.float64), 0.0)
        wi = np.where(usable, w * vis.imag.astype(np.float64), 0.0)
    shape = (C_out,) + vis.shape[1:]
    cov = np.zeros(shape, np.float64)
    S1 = np.zeros(shape, np.float64)
    S2 = np.zeros(shape, np.float64)
    Nr = np.zeros(shape, np.float64)
    Ni = np.zeros(shape, np.float64)
    for i in range(len(g)):
        # the output channels whose input i lies inside the band
        c = np.arange(C_out) * step - offset + i
        o = np.flatnonzero((c >= 0) & (c < C_in))
        c = c[o]
        gw = g[i] * w[c]
        cov[o] += np.where(usable[c], g[i], 0.0)
        S1[o] += gw
        S2[o] += g[i] * gw
        Nr[o] += g[i] * wr[c]
        Ni[o] += g[i] * wi[c]
    kept = cov >= min_sum
    with np.errstate(all='ignore'):
        out = np.zeros(shape, np.complex128)
        out.real = np.where(kept, Nr / S1, 0.0)
        out.imag = np.where(kept, Ni / S1, 0.0)
        new_weights = np.where(kept, (S1 * S1) / S2, 0.0)
    return out, new_weights, kept


def filter_host(vis, weights, params):
    """The contract of ``kimg_spectral_filter`` (include/kimg.h) in numpy: float64 until the final
    ``astype``.  ``vis`` complex64 and ``weights`` float32, both [C_in][N][Q].  Returns new arrays
    ``(vis, weights, (kept, flagged))`` with C_out channels."""
    out, new_weights, kept = filter_host_double(vis, weights, params)
    with np.errstate(all='ignore'):
        out = out.astype(np.complex64)
        new_weights = new_weights.astype(np.float32)
    n_kept = int(kept.sum())
    return out, new_weights, (n_kept, int(kept.size) - n_kept)


class SpectralFilter(ChannelOperator):
    """``kimg_spectral_filter`` for blocks of ``num_channels_in`` channels.  ``op(vis, weights)``
    reads two :class:`accel.DeviceArray` of shape [C_in][N][Q] (complex64 / float32) whose inner
    [N][Q] plane is dense -- the channel axis may have any pitch (a view of a larger tensor) -- and
    returns new dense device arrays ``(vis, weights)`` of shape [C_out][N][Q]; the inputs are left as
    they are.  The call is asynchronous on ``command_queue``.  :meth:`counts` reads back how many
    output samples have been kept and flagged since construction or :meth:`reset_counts`."""

    def __init__(self, template, command_queue, num_channels_in):
        params = template.params
        self.num_channels_out = params.output_channels(num_channels_in)
        super().__init__(template, command_queue, num_channels_in)
        self.num_channels_in = self.num_channels
        g, self._offset, self._step = params.coefficients()
        self._coeff = np.ascontiguousarray(g, np.float64)
        self._min_sum = params.min_sum()

    def __call__(self, vis, weights):
        self._check_block(vis, weights)
        queue = self.command_queue
        shape = (self.num_channels_out,) + tuple(vis.shape[1:])
        out_vis = accel.DeviceArray(queue.context, shape, np.complex64, queue=queue)
        out_weights = accel.DeviceArray(queue.context, shape, np.float32, queue=queue)
        plane = shape[1] * shape[2]
        if plane == 0:
            return out_vis, out_weights
        vis.used_on(queue)
        weights.used_on(queue)
        check(lib().kimg_spectral_filter(
            vis.ptr, channel_pitch(vis, 'vis'), weights.ptr,
            channel_pitch(weights, 'weights'), self.num_channels_in,
            out_vis.ptr, plane, out_weights.ptr, plane, self.num_channels_out, plane,
            self._coeff.ctypes.data_as(ctypes.c_void_p), len(self._coeff), self._offset, self._step,
            self._min_sum, self._counts.ptr, queue.handle), 'kimg_spectral_filter')
        return out_vis, out_weights


class SpectralFilterTemplate(OperatorTemplate):
    params_type = SpectralParameters
    operator = SpectralFilter
