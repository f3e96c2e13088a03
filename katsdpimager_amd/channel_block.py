"""What the operators on raw ``[channel][row][polarization]`` visibility blocks share
(:mod:`.continuum`, :mod:`.statwt`, :mod:`.rfiflag`, :mod:`.spectral`, :mod:`.phaseshift`; the device
side is csrc/kimg_channel_block.h): the layout and argument checks, the two spellings of a channel
selection, the groups of rows of one baseline, and the plumbing of a device operator and its
template.  The numpy twins and every operator's arithmetic stay in their own modules; this module
imports none of them.
"""
import numpy as np

from . import accel
from ._lib import lib

#: KIMG_UVCONTSUB_MAX_CHANNELS
MAX_CHANNELS = 16384
#: KIMG_STATWT_MAX_BIN
MAX_BIN = 64


def integer(value, name, low, high):
    """``value`` as an int, which it must be without loss, in ``low`` to ``high``."""
    try:
        as_int = int(value)
    except (TypeError, ValueError, OverflowError):
        raise ValueError('{} must be an integer'.format(name)) from None
    if as_int != value or not low <= as_int <= high:
        raise ValueError('{} must be an integer from {} to {}'.format(name, low, high))
    return as_int


def channel_count(num_channels):
    num_channels = int(num_channels)
    if num_channels < 1:
        raise ValueError('no channels')
    return num_channels


def channel_pitch(array, what):
    """Elements from one channel of a [C][N][Q] device array to the next.  The [N][Q] plane must be
    dense; the channel axis may have any pitch that keeps channels apart (a view of a larger
    tensor)."""
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


def check_block(vis, weights):
    """``vis`` complex64 and ``weights`` float32, both [channel][row][polarization] (numpy or device
    arrays)."""
    if vis.dtype != np.complex64 or weights.dtype != np.float32:
        raise TypeError('vis must be complex64 and weights float32')
    if len(vis.shape) != 3 or vis.shape != weights.shape:
        raise ValueError('vis and weights must both be [channel][row][polarization]')


class ChannelSelection:
    """Which channels of a band an operator works from, in two spellings: ``fit_mask`` (one entry
    per channel, nonzero = in) or ``line_ranges`` (a list of ``(first, last + 1)`` channel ranges
    left OUT).  ``order``: the degree of a polynomial to be fitted to the channels that are in --
    exactly one spelling must then be given and ``order + 1`` channels must remain -- or None: at
    most one spelling (with neither, every channel is in) and one channel must remain.  With
    ``line_ranges`` what remains is known only once the number of channels is (:meth:`mask`)."""

    def __init__(self, fit_mask=None, line_ranges=None, order=None):
        if order is not None and (fit_mask is None) == (line_ranges is None):
            raise ValueError('exactly one of fit_mask and line_ranges must be given')
        if fit_mask is not None and line_ranges is not None:
            raise ValueError('at most one of fit_mask and line_ranges may be given')
        self.order = order
        self.fit_mask = None
        self.line_ranges = None
        if fit_mask is not None:
            fit_mask = np.asarray(fit_mask)
            # (the fit reports an empty mask from mask(): 'no channels')
            if fit_mask.ndim != 1 or (order is None and not len(fit_mask)):
                raise ValueError('fit_mask must have one entry per channel')
            self.fit_mask = (fit_mask != 0).astype(np.uint8)
        elif line_ranges is not None:
            ranges = []
            for r in line_ranges:
                first, stop = (int(x) for x in r)
                if first < 0 or stop < first:
                    raise ValueError('bad line range {!r}'.format(r))
                ranges.append((first, stop))
            self.line_ranges = ranges

    def mask(self, num_channels):
        """The selection over ``num_channels`` channels, uint8 (1 = in)."""
        num_channels = channel_count(num_channels)
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
        if self.order is None:
            if not mask.any():
                raise ValueError('no line-free channel remains')
        elif int(mask.sum()) < self.order + 1:
            raise ValueError('order {} needs {} line-free channels, {} remain'.format(
                self.order, self.order + 1, int(mask.sum())))
        return mask

    def spelling(self, lead=''):
        """The keyword that was given, for a ``__repr__``: ``lead`` and ``fit_mask=[...]`` or
        ``line_ranges=[...]``, or nothing."""
        if self.fit_mask is not None:
            return '{}fit_mask={!r}'.format(lead, self.fit_mask.tolist())
        if self.line_ranges is not None:
            return '{}line_ranges={!r}'.format(lead, self.line_ranges)
        return ''


# ---- groups: up to time_bin consecutive rows of one baseline -------------------------------------
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


def group_tables(queue, baselines, num_rows, time_bin):
    """``(tables, G)`` of a block of ``num_rows`` rows with the HOST baseline ids ``baselines``:
    the group offsets [G + 1] and then the group of every row [N], int32, in one device array (one
    upload); ``tables`` is None for a block without rows."""
    baselines = np.asarray(baselines)
    if baselines.shape != (num_rows,) or baselines.dtype.kind not in 'iu':
        raise ValueError('baselines must be an integer array with one entry per row')
    offsets = group_offsets(baselines, time_bin)
    G = len(offsets) - 1
    if num_rows == 0:
        return None, G
    sizes = np.diff(offsets)
    if offsets[0] != 0 or offsets[-1] != num_rows or sizes.min() < 1 or sizes.max() > time_bin:
        raise ValueError('bad group offsets')
    host = np.concatenate((offsets, _row_groups(offsets)))
    tables = accel.DeviceArray(queue.context, host.shape, np.int32, queue=queue)
    tables.set(queue, host)
    return tables, G


def grown_workspace(queue, workspace, need):
    """``workspace`` (uint8 device array or None) if it holds ``need`` bytes, else a new one."""
    if workspace is None or workspace.shape[0] < need:
        workspace = accel.DeviceArray(queue.context, (need,), np.uint8, queue=queue)
    return workspace


# ---- the device operators ------------------------------------------------------------------------
class ChannelOperator:
    """What an operator made for blocks of ``num_channels`` channels on ``command_queue`` keeps:
    with ``masked``, the channel mask of its template's parameters (at most MAX_CHANNELS channels);
    its :attr:`COUNTERS` int64 counters on the device, which its kernels add to; and the checks of
    the blocks it is called with."""

    #: how many counters :meth:`counts` reads back
    COUNTERS = 2

    def __init__(self, template, command_queue, num_channels, masked=False):
        self.template = template
        self.command_queue = command_queue
        self.num_channels = int(num_channels)
        if masked:
            # ``template.params.mask`` as the host array the entry points take
            if self.num_channels > MAX_CHANNELS:
                raise ValueError('at most {} channels'.format(MAX_CHANNELS))
            self._mask = np.ascontiguousarray(template.params.mask(self.num_channels), np.uint8)
        self._counts = None
        if self.COUNTERS:
            self._counts = accel.DeviceArray(command_queue.context, (self.COUNTERS,), np.int64,
                                             queue=command_queue)
            self._counts.zero(command_queue)

    def _check_channels(self, vis):
        if vis.shape[0] != self.num_channels:
            raise ValueError('the operator was made for {} channels, the block has {}'.format(
                self.num_channels, vis.shape[0]))

    def _check_block(self, vis, weights):
        check_block(vis, weights)
        self._check_channels(vis)

    def counts(self):
        """The counters since construction or :meth:`reset_counts`, a tuple of ints (what they
        count is the operator's to say); waits for the queue."""
        return tuple(int(x) for x in self._counts.get(self.command_queue))

    def reset_counts(self):
        self._counts.zero(self.command_queue)


class OperatorTemplate:
    """``Template(context, params).instantiate(command_queue, ...)`` makes :attr:`operator`;
    ``params`` must be a :attr:`params_type`."""

    params_type = None
    operator = None

    def __init__(self, context, params, tuning=None):
        if not isinstance(params, self.params_type):
            raise TypeError('params must be ' + self.params_type.__name__)
        lib()
        self.context = context
        self.params = params

    def instantiate(self, *args, **kwargs):
        return self.operator(self, *args, **kwargs)
