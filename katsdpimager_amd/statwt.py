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
from .channel_block import (MAX_BIN, ChannelOperator, ChannelSelection, OperatorTemplate,
                            channel_pitch, check_block, group_offsets, group_tables,
                            grown_workspace, integer, _row_groups, _sum_over_groups)

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
        self.time_bin = integer(time_bin, 'time_bin', 1, MAX_BIN)
        self.min_samples = integer(min_samples, 'min_samples', 2, 2 ** 31 - 1)
        self._selection = ChannelSelection(fit_mask, line_ranges)
        self.fit_mask = self._selection.fit_mask
        self.line_ranges = self._selection.line_ranges
        if self.fit_mask is not None:
            self.mask(len(self.fit_mask))
        if chi2_range is None:
            chi2_range = (0.0, np.inf)
        try:
            lo, hi = (float(x) for x in chi2_range)
        except (TypeError, ValueError):
            raise ValueError('chi2_range must be two numbers') from None
        if not 0.0 <= lo < hi:                      # (false for NaN)
            raise ValueError('chi2_range must be (lo, hi) with 0 <= lo < hi')
        self.chi2_range = (lo, hi)

    def mask(self, num_channels):
        """The fit mask of ``num_channels`` channels, uint8 (1 = enters the statistic)."""
        return self._selection.mask(num_channels)

    def __repr__(self):
        return 'StatWtParameters({}{}, min_samples={}, chi2_range={!r})'.format(
            self.time_bin, self._selection.spelling(', '), self.min_samples, self.chi2_range)


def statwt_host(vis, weights, baselines, params):
    """The contract of ``kimg_statwt`` (include/kimg.h) in numpy, float64 throughout and every sum in
    the stated order: over channels in ascending order within a row, over rows in ascending order
    within a group.  ``vis`` complex64 and ``weights`` float32, both [C][N][P]; ``baselines`` [N].
    Returns ``(weights, chi2, (kept, flagged))``: new weights, chi2 float64 [G][P] (NaN where a group
    has fewer than 2 usable samples) and the counts in units of group x polarization."""
    vis = np.asarray(vis)
    weights = np.asarray(weights)
    check_block(vis, weights)
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


class StatWt(ChannelOperator):
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
        super().__init__(template, command_queue, num_channels, masked=True)
        params = template.params
        self.time_bin = params.time_bin
        self.min_samples = params.min_samples
        self.chi2_range = params.chi2_range
        self._workspace = None
        self._tables = None
        self.chi2 = None

    def __call__(self, vis, weights, baselines):
        self._check_block(vis, weights)
        C, N, P = vis.shape
        if not 1 <= P <= 4:
            raise ValueError('1 to 4 polarizations')
        queue = self.command_queue
        tables, G = group_tables(queue, baselines, N, self.time_bin)
        self.chi2 = accel.DeviceArray(queue.context, (G, P), np.float64, queue=queue)
        if N == 0:
            return
        self._tables = tables
        self._workspace = grown_workspace(queue, self._workspace, WORKSPACE_PER_ELEMENT * N * P)
        vis.used_on(queue)
        weights.used_on(queue)
        check(lib().kimg_statwt(
            vis.ptr, channel_pitch(vis, 'vis'), weights.ptr,
            channel_pitch(weights, 'weights'), C, N, P,
            self._mask.ctypes.data_as(ctypes.c_void_p), self._tables.ptr, G,
            self._tables.ptr + 4 * (G + 1), self.time_bin, self.min_samples,
            self.chi2_range[0], self.chi2_range[1], self.chi2.ptr, self._workspace.ptr,
            self._workspace.shape[0], self._counts.ptr, queue.handle), 'kimg_statwt')


class StatWtTemplate(OperatorTemplate):
    params_type = StatWtParameters
    operator = StatWt
