"""UV-plane continuum subtraction: a low-order polynomial fitted across the line-free channels of
every baseline sample and subtracted from all its channels (CASA's ``uvcontsub``, MIRIAD's
``uvlin``), on raw visibilities, ahead of preprocessing.

The reference removes continuum only through a sky model and the DFT predictor
(``Imaging.set_sky_model`` -> ``continuum_predict``); this is the route for calibrated
visibilities without a catalogue.  The contract is written in include/kimg.h ("UV-plane continuum
subtraction"); :func:`uvcontsub_host` is the same contract as numpy, and the executable
specification the device (csrc/contsub.hip, :class:`UVContSub`) is tested against.
``loader.preprocess_visibilities(..., continuum=UVContSubParameters(...))`` puts the operator
between the loader and the collector.
"""
import ctypes

import numpy as np

from . import accel
from ._lib import lib, check
from .channel_block import MAX_CHANNELS                                           # noqa: F401
from .channel_block import (ChannelOperator, ChannelSelection, OperatorTemplate, channel_count,
                            channel_pitch, check_block)

#: KIMG_UVCONTSUB_MAX_ORDER
MAX_ORDER = 3


class UVContSubParameters:
    """``order``: degree of the polynomial, 0 to 3.  Exactly one of ``fit_mask`` (one entry per
    channel, nonzero = a line-free channel that enters the fit) and ``line_ranges`` (a list of
    ``(first, last + 1)`` channel ranges left OUT of the fit) says which channels are line-free.
    ``frequencies`` (one per channel, optional): the polynomial is one in frequency instead of
    channel index.  At least ``order + 1`` channels must remain for the fit; with ``line_ranges``
    that is known only once the number of channels is (:meth:`mask`)."""

    def __init__(self, order, fit_mask=None, line_ranges=None, frequencies=None):
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
        self.frequencies = None
        if frequencies is not None:
            frequencies = np.asarray(frequencies, np.float64)
            if frequencies.ndim != 1 or not np.all(np.isfinite(frequencies)):
                raise ValueError('frequencies must be finite, one per channel')
            if self.fit_mask is not None and len(frequencies) != len(self.fit_mask):
                raise ValueError('fit_mask and frequencies differ in length')
            self.frequencies = frequencies
        if self.fit_mask is not None:
            self.mask(len(self.fit_mask))

    def mask(self, num_channels):
        """The fit mask of ``num_channels`` channels, uint8 (1 = enters the fit)."""
        num_channels = channel_count(num_channels)
        if self.frequencies is not None and len(self.frequencies) != num_channels:
            raise ValueError('{} frequencies for {} channels'.format(len(self.frequencies), num_channels))
        return self._selection.mask(num_channels)

    def __repr__(self):
        return 'UVContSubParameters({!r}, {}{})'.format(
            self.order, self._selection.spelling(),
            '' if self.frequencies is None else ', frequencies=...')


def legendre_basis(order, num_channels, frequencies=None):
    """float64 [order + 1][num_channels]: the Legendre polynomials P_0 .. P_order at x_c, where
    x_c = (2 c - (C - 1)) / (C - 1) runs from -1 at the first channel to 1 at the last (0 for a
    single channel), or, with ``frequencies``, the channel's frequency mapped linearly so that the
    lowest lies on -1 and the highest on 1 (0 where all are equal)."""
    if not 0 <= order <= MAX_ORDER or int(order) != order:
        raise ValueError('order must be an integer from 0 to {}'.format(MAX_ORDER))
    C = int(num_channels)
    if C < 1:
        raise ValueError('no channels')
    if frequencies is None:
        pos = np.arange(C, dtype=np.float64)
    else:
        pos = np.asarray(frequencies, np.float64)
        if pos.shape != (C,):
            raise ValueError('{} frequencies for {} channels'.format(pos.size, C))
    lo, hi = pos.min(), pos.max()
    # (distance from the low end) - (distance from the high end): exactly -1 and 1 at the ends
    x = ((pos - lo) - (hi - pos)) / (hi - lo) if hi > lo else np.zeros(C)
    basis = np.empty((int(order) + 1, C), np.float64)
    forms = (lambda x: np.ones_like(x), lambda x: x, lambda x: (3.0 * x * x - 1.0) / 2.0,
             lambda x: (5.0 * x * x - 3.0) * x / 2.0)
    for k in range(int(order) + 1):
        basis[k] = forms[k](x)
    return basis


def uvcontsub_host_double(vis, weights, params):
    """The contract up to its last step: (vis as complex128 BEFORE the one rounding to complex64,
    weights float32, fitted bool [N][Q]).  Where ``fitted`` is False the visibilities are the input's
    and the weights 0."""
    vis = np.asarray(vis)
    weights = np.asarray(weights)
    check_block(vis, weights)
    C = vis.shape[0]
    K = params.order + 1
    mask = params.mask(C)
    B = legendre_basis(params.order, C, params.frequencies)
    plane = vis.shape[1:]
    A = np.zeros((K, K) + plane, np.float64)
    b = np.zeros((K,) + plane, np.complex128)
    m = np.zeros(plane, np.int64)
    for c in range(C):
        if not mask[c]:
            continue
        usable = (weights[c] > 0) & np.isfinite(vis[c].real) & np.isfinite(vis[c].imag)
        w = np.where(usable, weights[c].astype(np.float64), 0.0)
        v = np.where(usable, vis[c].astype(np.complex128), 0.0)
        m += usable
        for k in range(K):
            wb = w * B[k, c]
            for l in range(k + 1):
                A[k, l] += wb * B[l, c]
            b[k] += wb * v
    fitted = m >= K
    with np.errstate(all='ignore'):
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
        out = vis.astype(np.complex128)
        for c in range(C):
            model = np.zeros(plane, np.complex128)
            for k in range(K):
                model += a[k] * B[k, c]
            out[c] = np.where(fitted, out[c] - model, out[c])
    new_weights = np.where(fitted[np.newaxis], weights, np.float32(0.0)).astype(np.float32)
    return out, new_weights, fitted


def uvcontsub_host(vis, weights, params):
    """The contract of ``kimg_uvcontsub`` (include/kimg.h) in numpy: float64 until the final
    ``astype(complex64)``.  ``vis`` complex64 and ``weights`` float32, both [C][N][Q].  Returns new
    arrays ``(vis, weights, (fitted, flagged))``."""
    out, new_weights, fitted = uvcontsub_host_double(vis, weights, params)
    with np.errstate(all='ignore'):
        rounded = out.astype(np.complex64)
    # (samples that could not be fitted keep their visibilities bit for bit, NaN payloads included)
    rounded = np.where(fitted[np.newaxis], rounded, np.asarray(vis))
    n_fitted = int(fitted.sum())
    return rounded, new_weights, (n_fitted, int(fitted.size) - n_fitted)


class UVContSub(ChannelOperator):
    """``kimg_uvcontsub`` for blocks of ``num_channels`` channels.  ``op(vis, weights)`` works in
    place on two :class:`accel.DeviceArray` of shape [C][N][Q] (complex64 / float32) whose inner
    [N][Q] plane is dense; the channel axis may have any pitch (a view of a larger tensor).  The
    call is asynchronous on ``command_queue``.  :meth:`counts` reads back how many samples have been
    fitted and flagged since construction or :meth:`reset_counts`."""

    def __init__(self, template, command_queue, num_channels):
        super().__init__(template, command_queue, num_channels, masked=True)
        params = template.params
        self.order = params.order
        basis = legendre_basis(params.order, self.num_channels, params.frequencies)
        self._basis = accel.DeviceArray(command_queue.context, basis.shape, np.float64,
                                        queue=command_queue)
        self._basis.set(command_queue, basis)

    def __call__(self, vis, weights):
        self._check_block(vis, weights)
        plane = vis.shape[1] * vis.shape[2]
        if plane == 0:
            return
        vis.used_on(self.command_queue)
        weights.used_on(self.command_queue)
        check(lib().kimg_uvcontsub(
            vis.ptr, channel_pitch(vis, 'vis'), weights.ptr,
            channel_pitch(weights, 'weights'), self.num_channels, plane,
            self._mask.ctypes.data_as(ctypes.c_void_p), self._basis.ptr, self.order,
            self._counts.ptr, self.command_queue.handle), 'kimg_uvcontsub')


class UVContSubTemplate(OperatorTemplate):
    params_type = UVContSubParameters
    operator = UVContSub
