"""RFI flagging: interference found in the time-frequency plane of every baseline by SumThreshold
(AOFlagger; CASA's ``flagdata mode='tfcrop'`` / ``'rflag'`` with ``extendflags``) and taken out of
raw visibilities by zeroing their weights, ahead of preprocessing.

Every operator of the raw-block chain reads a positive weight as "this sample is good", and
``statwt``'s ``chi2_range`` can only cut whole groups.  This operator decides per sample.  Per group
of up to ``time_bin`` consecutive rows of one baseline and per polarization it takes the plane of
``z = w |v|^2`` (channels x rows), measures its level as a clipped mean over the line-free channels
and runs SumThreshold over ``z - level``: windows of 1, 2, 4, ... samples along frequency and along
time whose sum exceeds the window's (falling) threshold are flagged, an already flagged sample
counting as exactly the threshold.  (For noise ``z`` is exponentially distributed: its mean AND its
scatter are the level, so thresholds in units of the level are thresholds in sigma about zero, what
SumThreshold's factors are made for.)  The flags are then extended over rows, channels and
polarizations that are mostly flagged already.  Line channels are protected: a bright line is constant in time and would
be flagged otherwise; only the extension over a row can reach them.  Flagged samples get a weight of
+0.0; nothing else is written, the visibilities never.

The contract is written in include/kimg.h ("RFI flagging"); :func:`rfiflag_host` is the same
contract as numpy, and the executable specification the device (csrc/rfiflag.hip, :class:`RFIFlag`)
matches bit for bit.  ``loader.preprocess_visibilities(..., rfiflag=RFIFlagParameters())`` puts the
operator between the continuum fit and ``statwt``.

Not done: a surface-fit high-pass of the plane (the level is one number per group), medians or other
order statistics, groups across block boundaries (a baseline's rows in the next loader block start
new groups), re-running the continuum fit on the flagged residuals.
"""
import ctypes

import numpy as np

from . import accel
from ._lib import lib, check
from .channel_block import (MAX_BIN, ChannelOperator, ChannelSelection, OperatorTemplate,
                            channel_pitch, check_block, group_offsets, group_tables,
                            grown_workspace, integer, _row_groups, _sum_over_groups)

#: KIMG_RFIFLAG_MAX_WINDOW
MAX_WINDOW = 32
#: KIMG_RFIFLAG_MAX_LEVEL_ITERATIONS
MAX_LEVEL_ITERATIONS = 4
#: KIMG_RFIFLAG_WORKSPACE_PER_ELEMENT (per sample: z as float64 and one byte of flag state)
WORKSPACE_PER_ELEMENT = 9
#: KIMG_RFIFLAG_WORKSPACE_PER_ROW (per element of the [row][polarization] plane: two sets of the
#: level's per-row partial sums, a float64 and an int32 each)
WORKSPACE_PER_ROW = 24
#: KIMG_RFIFLAG_TIME, KIMG_RFIFLAG_FREQ
DIRECTIONS = {'time': 1, 'freq': 2, 'both': 3}


class RFIFlagParameters:
    """``time_bin``: rows of one baseline per group (the plane's time axis), 1 to 64.  ``threshold``
    (> 0) and ``rho`` (>= 1): a window of ``m = 2**k`` samples is flagged if the mean of its
    ``z - level`` exceeds ``threshold / rho**k`` times the level; ``max_window``: the longest
    window, a power of two from 1 to 32.  ``directions``: ``'time'``, ``'freq'`` or ``'both'``.  ``level_iterations`` (0 to 4) and
    ``level_clip`` (> 0): the level is the mean of ``z``, then that many times the mean of the
    samples not above ``level_clip`` times the previous one.  ``extend_freq``, ``extend_time``: a
    fraction in (0, 1], or None for no extension: a row (a channel of a group) with more than that
    share of its usable samples flagged is flagged entirely.  ``extend_pols``: a sample flagged in
    one polarization is flagged in all.  At most one of ``fit_mask`` and ``line_ranges``, as for
    :class:`~.statwt.StatWtParameters`: the channels left out are protected."""

    def __init__(self, time_bin=64, threshold=6.0, rho=1.5, max_window=16, directions='both',
                 level_iterations=2, level_clip=4.0, extend_freq=0.5, extend_time=0.5,
                 extend_pols=True, fit_mask=None, line_ranges=None):
        self.time_bin = integer(time_bin, 'time_bin', 1, MAX_BIN)
        self.max_window = integer(max_window, 'max_window', 1, MAX_WINDOW)
        if self.max_window & (self.max_window - 1):
            raise ValueError('max_window must be a power of two')
        self.level_iterations = integer(level_iterations, 'level_iterations', 0, MAX_LEVEL_ITERATIONS)
        self.threshold = self._number(threshold, 'threshold')
        self.rho = self._number(rho, 'rho')
        self.level_clip = self._number(level_clip, 'level_clip')
        if not (0.0 < self.threshold < np.inf):                 # (false for NaN)
            raise ValueError('threshold must be positive and finite')
        if not (1.0 <= self.rho < np.inf):
            raise ValueError('rho must be at least 1 and finite')
        if not (0.0 < self.level_clip < np.inf):
            raise ValueError('level_clip must be positive and finite')
        if directions not in DIRECTIONS:
            raise ValueError("directions must be 'time', 'freq' or 'both'")
        self.directions = directions
        self.extend_freq = self._fraction(extend_freq, 'extend_freq')
        self.extend_time = self._fraction(extend_time, 'extend_time')
        if not isinstance(extend_pols, (bool, np.bool_)):
            raise ValueError('extend_pols must be True or False')
        self.extend_pols = bool(extend_pols)
        self._selection = ChannelSelection(fit_mask, line_ranges)
        self.fit_mask = self._selection.fit_mask
        self.line_ranges = self._selection.line_ranges
        if self.fit_mask is not None:
            self.mask(len(self.fit_mask))

    @staticmethod
    def _number(value, name):
        if isinstance(value, (bool, np.bool_)):
            raise ValueError('{} must be a number'.format(name))
        try:
            return float(value)
        except (TypeError, ValueError):
            raise ValueError('{} must be a number'.format(name)) from None

    @classmethod
    def _fraction(cls, value, name):
        if value is None:
            return None
        value = cls._number(value, name)
        if not (0.0 < value <= 1.0):                            # (false for NaN)
            raise ValueError('{} must be None or lie in (0, 1]'.format(name))
        return value

    def mask(self, num_channels):
        """The channel mask of ``num_channels`` channels, uint8 (1 = searched for interference and
        part of the level, 0 = protected)."""
        return self._selection.mask(num_channels)

    def factors(self):
        """float64 [log2(max_window) + 1]: ``threshold / rho**k``, the threshold of a window of
        ``2**k`` samples per sample, in units of the level."""
        k = np.arange(self.max_window.bit_length(), dtype=np.float64)
        return np.float64(self.threshold) / np.float64(self.rho) ** k

    def __repr__(self):
        return ('RFIFlagParameters({}, threshold={!r}, rho={!r}, max_window={}, directions={!r}, '
                'level_iterations={}, level_clip={!r}, extend_freq={!r}, extend_time={!r}, '
                'extend_pols={!r}{})').format(
                    self.time_bin, self.threshold, self.rho, self.max_window, self.directions,
                    self.level_iterations, self.level_clip, self.extend_freq, self.extend_time,
                    self.extend_pols, self._selection.spelling(', '))


def rfiflag_host(vis, weights, baselines, params):
    """The contract of ``kimg_rfi_flag`` (include/kimg.h) in numpy, float64 throughout and every sum
    in the stated order.  ``vis`` complex64 and ``weights`` float32, both [C][N][P]; ``baselines``
    [N].  Returns ``(weights, flags, level, (kept, flagged, skipped))``: new weights, flags uint8
    [C][N][P], the level float64 [G][P] (NaN where the pair was skipped) and the counts: usable
    samples kept and flagged, and skipped (group, polarization) pairs."""
    vis = np.asarray(vis)
    weights = np.asarray(weights)
    check_block(vis, weights)
    C, N, P = vis.shape
    if len(baselines) != N:
        raise ValueError('{} baselines for {} rows'.format(len(baselines), N))
    if not 1 <= P <= 4:
        raise ValueError('1 to 4 polarizations')
    mask = params.mask(C) != 0
    offsets = group_offsets(baselines, params.time_bin)
    G = len(offsets) - 1
    if N == 0:
        return weights.copy(), np.zeros((C, 0, P), np.uint8), np.zeros((0, P), np.float64), (0, 0, 0)
    row_group = _row_groups(offsets)
    stop = offsets[1:].astype(np.int64)[row_group]              # one past the last row of a row's group
    T = params.time_bin
    fit = np.flatnonzero(mask)

    with np.errstate(all='ignore'):
        re = vis.real.astype(np.float64)
        im = vis.imag.astype(np.float64)
        usable = (weights > 0) & np.isfinite(weights) & np.isfinite(vis.real) & np.isfinite(vis.imag)
        t = re * re
        t = t + im * im
        z = weights.astype(np.float64) * t
        search = usable & mask[:, None, None]                   # usable samples of mask channels

        # ---- the level: a clipped mean per (group, polarization)
        def mean(select):
            zrow = np.zeros((N, P), np.float64)
            mrow = np.zeros((N, P), np.int64)
            for c in fit:
                zrow = np.where(select[c], zrow + z[c], zrow)
                mrow += select[c]
            Z = _sum_over_groups(zrow, offsets, T)
            M = _sum_over_groups(mrow, offsets, T)
            L = Z / M.astype(np.float64)
            return L, (M > 0) & np.isfinite(L) & (L > 0)
        L, alive = mean(search)
        for _ in range(params.level_iterations):
            limit = np.float64(params.level_clip) * L
            L, ok = mean(search & (z <= limit[row_group][None]) & alive[row_group][None])
            alive &= ok
        level = np.where(alive, L, np.nan)
        Lrow = level[row_group][None]                           # [1][N][P]; NaN: nothing compares true

        # ---- SumThreshold
        flags = np.zeros((C, N, P), bool)
        for k, factor in enumerate(params.factors()):
            m = 1 << k
            chi = np.float64(factor) * Lrow
            limit = np.float64(m) * chi
            good = search & ~flags
            a = np.where(good, z - Lrow, np.broadcast_to(chi, z.shape))
            new = np.zeros_like(flags)
            if params.directions in ('freq', 'both') and m <= C:
                W = C - m + 1
                acc = np.zeros((W, N, P), np.float64)
                any_good = np.zeros((W, N, P), bool)
                for i in range(m):
                    acc = acc + a[i:i + W]
                    any_good |= good[i:i + W]
                hit = any_good & (acc > limit)
                for i in range(m):
                    new[i:i + W] |= hit
            if params.directions in ('time', 'both') and m <= N:
                W = N - m + 1
                acc = np.zeros((C, W, P), np.float64)
                any_good = np.zeros((C, W, P), bool)
                for i in range(m):
                    acc = acc + a[:, i:i + W]
                    any_good |= good[:, i:i + W]
                inside = np.arange(W) + m <= stop[:W]           # the window stays in its group
                hit = any_good & (acc > limit[:, :W]) & inside[None, :, None]
                for i in range(m):
                    new[:, i:i + W] |= hit
            flags |= new & search

        # ---- extension
        alive_row = alive[row_group][None]                      # [1][N][P]
        if params.extend_freq is not None:
            have = search.sum(axis=0).astype(np.float64)        # [N][P]
            hit = (flags & search).sum(axis=0).astype(np.float64)
            flags |= (hit > np.float64(params.extend_freq) * have)[None] & alive_row & usable
        if params.extend_time is not None:
            per_row = np.moveaxis(search, 0, 1).astype(np.int64)            # [N][C][P]
            have = _sum_over_groups(per_row, offsets, T).astype(np.float64)  # [G][C][P]
            per_row = np.moveaxis(flags & search, 0, 1).astype(np.int64)
            hit = _sum_over_groups(per_row, offsets, T).astype(np.float64)
            whole = hit > np.float64(params.extend_time) * have
            flags |= np.moveaxis(whole[row_group], 0, 1) & search
        if params.extend_pols:
            flags |= flags.any(axis=2, keepdims=True) & alive_row & usable
    new_weights = np.where(flags, np.float32(0.0), weights).astype(np.float32)
    flagged = int(flags.sum())
    counts = (int(usable.sum()) - flagged, flagged, int(alive.size - alive.sum()))
    return new_weights, flags.astype(np.uint8), level, counts


class RFIFlag(ChannelOperator):
    """``kimg_rfi_flag`` for blocks of ``num_channels`` channels.  ``op(vis, weights, baselines)``
    zeroes the weights of the samples it flags and leaves ``vis`` alone: two
    :class:`accel.DeviceArray` of shape [C][N][P] (complex64 / float32) whose inner [N][P] plane is
    dense -- the channel axis may have any pitch -- and a HOST integer array [N] of the rows'
    baseline ids, from which the groups are made here (:func:`~.statwt.group_offsets`) and uploaded.
    The call is asynchronous on ``command_queue`` once the group tables are on the device.
    :attr:`flags` (uint8 [C][N][P]) and :attr:`level` (float64 [G][P]) are the last call's, device
    arrays (None before the first call); :meth:`counts` reads back the usable samples kept and
    flagged and the (group, polarization) pairs skipped since construction or :meth:`reset_counts`.
    The workspace is the operator's and grows on demand."""

    COUNTERS = 3

    def __init__(self, template, command_queue, num_channels):
        super().__init__(template, command_queue, num_channels, masked=True)
        params = template.params
        self.params = params
        self.time_bin = params.time_bin
        self._factors = np.ascontiguousarray(params.factors(), np.float64)
        self._workspace = None
        self._tables = None
        self.flags = None
        self.level = None

    @staticmethod
    def workspace_bytes(C, N, P):
        return WORKSPACE_PER_ELEMENT * C * N * P + WORKSPACE_PER_ROW * N * P

    def __call__(self, vis, weights, baselines):
        self._check_block(vis, weights)
        C, N, P = vis.shape
        if not 1 <= P <= 4:
            raise ValueError('1 to 4 polarizations')
        queue = self.command_queue
        context = queue.context
        tables, G = group_tables(queue, baselines, N, self.time_bin)
        self.flags = accel.DeviceArray(context, (C, N, P), np.uint8, queue=queue)
        self.level = accel.DeviceArray(context, (G, P), np.float64, queue=queue)
        if N == 0:
            return
        self._tables = tables
        self._workspace = grown_workspace(queue, self._workspace, self.workspace_bytes(C, N, P))
        vis.used_on(queue)
        weights.used_on(queue)
        params = self.params
        check(lib().kimg_rfi_flag(
            vis.ptr, channel_pitch(vis, 'vis'), weights.ptr,
            channel_pitch(weights, 'weights'), C, N, P,
            self._mask.ctypes.data_as(ctypes.c_void_p), self._tables.ptr, G,
            self._tables.ptr + 4 * (G + 1), self.time_bin,
            self._factors.ctypes.data_as(ctypes.c_void_p), params.max_window,
            DIRECTIONS[params.directions], params.level_iterations, params.level_clip,
            0.0 if params.extend_freq is None else params.extend_freq,
            0.0 if params.extend_time is None else params.extend_time,
            int(params.extend_pols), self.flags.ptr, self.level.ptr, self._workspace.ptr,
            self._workspace.shape[0], self._counts.ptr, queue.handle), 'kimg_rfi_flag')


class RFIFlagTemplate(OperatorTemplate):
    params_type = RFIFlagParameters
    operator = RFIFlag
