"""Statistical reweighting: the weights of raw visibilities rescaled to inverse variances measured
from the scatter of the visibilities themselves across the line-free channels (CASA's ``statwt``,
which CASA's spectral-line guides run after ``uvcontsub`` and before imaging), ahead of
preprocessing.

Correlator weights are relative at best, and everything downstream -- robust weighting, the uv taper,
``normalized_noise``, the CLEAN threshold, the auto-mask's sigma -- reads them as absolute inverse
variances.  Per group of up to ``time_bin`` consecutive rows of one baseline and per polarization the
operator measures chi2, the weighted scatter per real component about the group's own mean, and
divides every weight of the group by it: relative channel weights survive (they matter after the
spectral filter, whose outputs carry different weights), only the absolute scale is measured.  The
contract is written in include/kimg.h ("Statistical reweighting"); :func:`statwt_host` is the same
contract as numpy, and the executable specification the device (csrc/statwt.hip, :class:`StatWt`)
matches bit for bit.  ``loader.preprocess_visibilities(..., statwt=StatWtParameters(8))`` puts the
operator between the continuum fit and the collector.

Not done: pooling polarizations, channel bins narrower than the band, groups across block boundaries
(a baseline's rows in the next loader block start new groups), sliding windows, medians or other
robust statistics.
"""
import ctypes

import numpy as np

from . import accel
from ._lib import lib, check
from .continuum import MAX_CHANNELS

#: KIMG_STATWT_MAX_BIN
MAX_BIN = 64
#: KIMG_STATWT_WORKSPACE_PER_ELEMENT
WORKSPACE_PER_ELEMENT = 36


class StatWtParameters:
    """``time_bin``: rows of one baseline per group, 1 to 64.  At most one of ``fit_mask`` (one entry
    per channel, nonzero = a line-free channel that enters the statistic) and ``line_ranges`` (a list
    of ``(first, last + 1)`` channel ranges left OUT of it), the two spellings of
    :class:`~.continuum.UVContSubParameters`; with neither, every channel enters.  ``min_samples``
    (at least 2): a group with fewer usable samples is flagged.  ``chi2_range`` = (lo, hi),
    0 <= lo < hi, default (0, inf): a group is kept only if lo < chi2 < hi -- the outlier cut (CASA's
    ``wtrange``, stated on the variance)."""

    def __init__(self, time_bin=1, fit_mask=None, line_ranges=None, min_samples=8, chi2_range=None):
        self.time_bin = self._integer(time_bin, 'time_bin', 1, MAX_BIN)
        self.min_samples = self._integer(min_samples, 'min_samples', 2, 2 ** 31 - 1)
        if fit_mask is not None and line_ranges is not None:
            raise ValueError('at most one of fit_mask and line_ranges may be given')
        self.fit_mask = None
        self.line_ranges = None
        if fit_mask is not None:
            fit_mask = np.asarray(fit_mask)
            if fit_mask.ndim != 1 or not len(fit_mask):
                raise ValueError('fit_mask must have one entry per channel')
            self.fit_mask = (fit_mask != 0).astype(np.uint8)
            self.mask(len(self.fit_mask))
        elif line_ranges is not None:
            ranges = []
            for r in line_ranges:
                first, stop = (int(x) for x in r)
                if first < 0 or stop < first:
                    raise ValueError('bad line range {!r}'.format(r))
                ranges.append((first, stop))
            self.line_ranges = ranges
        if chi2_range is None:
            chi2_range = (0.0, np.inf)
        try:
            lo, hi = (float(x) for x in chi2_range)
        except (TypeError, ValueError):
            raise ValueError('chi2_range must be two numbers') from None
        if not 0.0 <= lo < hi:                      # (false for NaN)
            raise ValueError('chi2_range must be (lo, hi) with 0 <= lo < hi')
        self.chi2_range = (lo, hi)

    @staticmethod
    def _integer(value, name, low, high):
        try:
            as_int = int(value)
        except (TypeError, ValueError, OverflowError):
            raise ValueError('{} must be an integer'.format(name)) from None
        if as_int != value or not low <= as_int <= high:
            raise ValueError('{} must be an integer from {} to {}'.format(name, low, high))
        return as_int

    def mask(self, num_channels):
        """The fit mask of ``num_channels`` channels, uint8 (1 = enters the statistic)."""
        num_channels = int(num_channels)
        if num_channels < 1:
            raise ValueError('no channels')
        if self.fit_mask is not None:
            if len(self.fit_mask) != num_channels:
                raise ValueError('fit_mask has {} entries for {} channels'.format(
                    len(self.fit_mask), num_channels))
            mask = self.fit_mask.copy()
        else:
            mask = np.ones(num_channels, np.uint8)
            for first, stop in self.line_ranges or ():
                if stop > num_channels:
                    raise ValueError('line range ({}, {}) beyond the {} channels'.format(
                        first, stop, num_channels))
                mask[first:stop] = 0
        if not mask.any():
            raise ValueError('no line-free channel remains')
        return mask

    def __repr__(self):
        which = ''
        if self.fit_mask is not None:
            which = ', fit_mask={!r}'.format(self.fit_mask.tolist())
        elif self.line_ranges is not None:
            which = ', line_ranges={!r}'.format(self.line_ranges)
        return 'StatWtParameters({}{}, min_samples={}, chi2_range={!r})'.format(
            self.time_bin, which, self.min_samples, self.chi2_range)


def group_offsets(baselines, time_bin):
    """int32 [G + 1]: the first row of every group of a block whose rows carry the baseline ids
    ``baselines`` [N], and N at the end.  Equal consecutive ids form a run (an id that returns later
    in the block starts a new run); each run is cut every ``time_bin`` rows, its last group taking
    what is left."""
    baselines = np.asarray(baselines)
    if baselines.ndim != 1:
        raise ValueError('baselines must have one entry per row')
    time_bin = int(time_bin)
    if not 1 <= time_bin <= MAX_BIN:
        raise ValueError('time_bin must lie in 1 to {}'.format(MAX_BIN))
    N = len(baselines)
    if N > 2 ** 31 - 1:
        raise ValueError('too many rows')
    if N == 0:
        return np.zeros(1, np.int32)
    starts = np.flatnonzero(np.concatenate(([True], baselines[1:] != baselines[:-1])))
    lengths = np.diff(np.concatenate((starts, [N])))
    groups = (lengths + time_bin - 1) // time_bin           # per run
    run = np.repeat(np.arange(len(starts)), groups)         # per group
    within = np.arange(int(groups.sum())) - (np.cumsum(groups) - groups)[run]
    return np.concatenate((starts[run] + within * time_bin, [N])).astype(np.int32)


def _row_groups(offsets):
    """int32 [N]: the group of every row."""
    return np.repeat(np.arange(len(offsets) - 1, dtype=np.int32), np.diff(offsets))


def _sum_over_groups(per_row, offsets, time_bin):
    """[G][P]: the rows of every group added up in ascending row order, starting from 0."""
    first, stop = offsets[:-1].astype(np.int64), offsets[1:].astype(np.int64)
    total = np.zeros((len(first),) + per_row.shape[1:], per_row.dtype)
    for i in range(time_bin):
        has = first + i < stop
        total[has] = total[has] + per_row[first[has] + i]
    return total


def statwt_host(vis, weights, baselines, params):
    """The contract of ``kimg_statwt`` (include/kimg.h) in numpy, float64 throughout and every sum in
    the stated order: over channels in ascending order within a row, over rows in ascending order
    within a group.  ``vis`` complex64 and ``weights`` float32, both [C][N][P]; ``baselines`` [N].
    Returns ``(weights, chi2, (kept, flagged))``: new weights, chi2 float64 [G][P] (NaN where a group
    has fewer than 2 usable samples) and the counts in units of group x polarization."""
    vis = np.asarray(vis)
    weights = np.asarray(weights)
    if vis.dtype != np.complex64 or weights.dtype != np.float32:
        raise TypeError('vis must be complex64 and weights float32')
    if vis.ndim != 3 or vis.shape != weights.shape:
        raise ValueError('vis and weights must both be [channel][row][polarization]')
    C, N, P = vis.shape
    if len(baselines) != N:
        raise ValueError('{} baselines for {} rows'.format(len(baselines), N))
    mask = params.mask(C)
    offsets = group_offsets(baselines, params.time_bin)
    row_group = _row_groups(offsets)
    lo, hi = params.chi2_range
    fit = [c for c in range(C) if mask[c]]

    def sample(c):
        usable = (weights[c] > 0) & np.isfinite(weights[c]) \
            & np.isfinite(vis[c].real) & np.isfinite(vis[c].imag)
        return (usable, weights[c].astype(np.float64), vis[c].real.astype(np.float64),
                vis[c].imag.astype(np.float64))
    with np.errstate(all='ignore'):
        # 1. per row, over its usable channels
        s0 = np.zeros((N, P), np.float64)
        sr = np.zeros((N, P), np.float64)
        si = np.zeros((N, P), np.float64)
        m = np.zeros((N, P), np.int64)
        for c in fit:
            usable, w, re, im = sample(c)
            s0 = np.where(usable, s0 + w, s0)
            sr = np.where(usable, sr + w * re, sr)
            si = np.where(usable, si + w * im, si)
            m += usable
        # 2. over the group's rows; the mean
        S0 = _sum_over_groups(s0, offsets, params.time_bin)
        SR = _sum_over_groups(sr, offsets, params.time_bin)
        SI = _sum_over_groups(si, offsets, params.time_bin)
        M = _sum_over_groups(m, offsets, params.time_bin)
        mu_r = (SR / S0)[row_group]
        mu_i = (SI / S0)[row_group]
        # 3. the scatter about it
        q = np.zeros((N, P), np.float64)
        for c in fit:
            usable, w, re, im = sample(c)
            dr = re - mu_r
            di = im - mu_i
            t = dr * dr
            t = t + di * di
            q = np.where(usable, q + w * t, q)
        Q = _sum_over_groups(q, offsets, params.time_bin)
        # 4., 5.
        chi2 = Q / (2.0 * (M - 1).astype(np.float64))
        kept = (M >= params.min_samples) & (lo < chi2) & (chi2 < hi)
        scaled = (weights.astype(np.float64) / chi2[row_group][np.newaxis]).astype(np.float32)
    new_weights = np.where(kept[row_group][np.newaxis], np.where(weights > 0, scaled, weights),
                           np.float32(0.0)).astype(np.float32)
    n_kept = int(kept.sum())
    return new_weights, np.where(M < 2, np.nan, chi2), (n_kept, int(kept.size) - n_kept)


class StatWtTemplate:
    def __init__(self, context, params, tuning=None):
        if not isinstance(params, StatWtParameters):
            raise TypeError('params must be StatWtParameters')
        lib()
        self.context = context
        self.params = params

    def instantiate(self, *args, **kwargs):
        return StatWt(self, *args, **kwargs)


class StatWt:
    """``kimg_statwt`` for blocks of ``num_channels`` channels.  ``op(vis, weights, baselines)``
    rescales ``weights`` in place and leaves ``vis`` alone: two :class:`accel.DeviceArray` of shape
    [C][N][P] (complex64 / float32) whose inner [N][P] plane is dense -- the channel axis may have
    any pitch (a view of a larger tensor) -- and a HOST integer array [N] of the rows' baseline ids,
    from which the groups are made here (:func:`group_offsets`) and uploaded.  The call is
    asynchronous on ``command_queue`` once the group tables are on the device.  :meth:`counts` reads
    back how many (group, polarization) pairs have been kept and flagged since construction or
    :meth:`reset_counts`; :attr:`chi2` is the last call's chi2, a device array [G][P] (None before
    the first call).  The workspace is the operator's and grows on demand."""

    def __init__(self, template, command_queue, num_channels):
        params = template.params
        self.template = template
        self.command_queue = command_queue
        self.num_channels = int(num_channels)
        if self.num_channels > MAX_CHANNELS:
            raise ValueError('at most {} channels'.format(MAX_CHANNELS))
        self.time_bin = params.time_bin
        self.min_samples = params.min_samples
        self.chi2_range = params.chi2_range
        self._mask = np.ascontiguousarray(params.mask(self.num_channels), np.uint8)
        self._counts = accel.DeviceArray(command_queue.context, (2,), np.int64, queue=command_queue)
        self._counts.zero(command_queue)
        self._workspace = None
        self._tables = None
        self.chi2 = None

    @staticmethod
    def _channel_pitch(array, what):
        t = array.tensor
        C, N, Q = array.shape
        if N * Q == 0:
            return 0
        strides = t.stride()
        if (Q > 1 and strides[2] != 1) or (N > 1 and strides[1] != Q):
            raise ValueError('{}: the [row][polarization] plane must be dense'.format(what))
        if C == 1:
            return N * Q
        if strides[0] < N * Q:
            raise ValueError('{}: channels overlap'.format(what))
        return int(strides[0])

    def __call__(self, vis, weights, baselines):
        if vis.dtype != np.complex64 or weights.dtype != np.float32:
            raise TypeError('vis must be complex64 and weights float32')
        if len(vis.shape) != 3 or vis.shape != weights.shape:
            raise ValueError('vis and weights must both be [channel][row][polarization]')
        if vis.shape[0] != self.num_channels:
            raise ValueError('the operator was made for {} channels, the block has {}'.format(
                self.num_channels, vis.shape[0]))
        C, N, P = vis.shape
        if not 1 <= P <= 4:
            raise ValueError('1 to 4 polarizations')
        baselines = np.asarray(baselines)
        if baselines.shape != (N,) or baselines.dtype.kind not in 'iu':
            raise ValueError('baselines must be an integer array with one entry per row')
        queue = self.command_queue
        context = queue.context
        offsets = group_offsets(baselines, self.time_bin)
        G = len(offsets) - 1
        self.chi2 = accel.DeviceArray(context, (G, P), np.float64, queue=queue)
        if N == 0:
            return
        sizes = np.diff(offsets)
        if offsets[0] != 0 or offsets[-1] != N or sizes.min() < 1 or sizes.max() > self.time_bin:
            raise ValueError('bad group offsets')
        # one upload: the offsets, then the group of every row
        tables = np.concatenate((offsets, _row_groups(offsets)))
        self._tables = accel.DeviceArray(context, tables.shape, np.int32, queue=queue)
        self._tables.set(queue, tables)
        need = WORKSPACE_PER_ELEMENT * N * P
        if self._workspace is None or self._workspace.shape[0] < need:
            self._workspace = accel.DeviceArray(context, (need,), np.uint8, queue=queue)
        vis.used_on(queue)
        weights.used_on(queue)
        check(lib().kimg_statwt(
            vis.ptr, self._channel_pitch(vis, 'vis'), weights.ptr,
            self._channel_pitch(weights, 'weights'), C, N, P,
            self._mask.ctypes.data_as(ctypes.c_void_p), self._tables.ptr, G,
            self._tables.ptr + 4 * (G + 1), self.time_bin, self.min_samples,
            self.chi2_range[0], self.chi2_range[1], self.chi2.ptr, self._workspace.ptr,
            self._workspace.shape[0], self._counts.ptr, queue.handle), 'kimg_statwt')

    def counts(self):
        """(kept, flagged) group x polarization pairs so far; waits for the queue."""
        host = self._counts.get(self.command_queue)
        return int(host[0]), int(host[1])

    def reset_counts(self):
        self._counts.zero(self.command_queue)
