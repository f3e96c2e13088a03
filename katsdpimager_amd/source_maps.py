"""Per-source moment maps: the moment maps of every source that :mod:`.link` has found, each inside its
own bounding box -- what SoFiA writes next to its catalogue and what CASA users build per region with
``immoments`` -- in ONE pass over labels and cube, whatever the number of sources.

:class:`SourceMapsTemplate` / :class:`SourceMapper` is the operator on the device
(csrc/cube_source_maps.hip: ``kimg_cube_source_maps``, ``kimg_source_maps_finish``).  ``op(labels,
the_cube, catalogue)`` takes the :class:`link.LabelCube` and the catalogue of one :class:`link.Link` call
and returns a :class:`SourceMaps`: ragged device tables with one entry per (source, pixel of its box) for
every moment asked for and ``'count'``.  The route this replaces is ``labels.mask(source=k)``,
:meth:`detect.MaskCube.apply` and :class:`cube.Moments` with ``channels=(c0, c1 + 1)``: three passes over
the cube per source.  :func:`source_maps_host` is the contract as numpy, the executable specification;
:func:`source_rows` makes the per-source table both take.

The contract (include/kimg.h, "Per-source moment maps").

* ``rows`` (:data:`ROW_DTYPE`, a row per source 1 to N): ``offset``, ``pol``, the box ``y0, x0, h, w``,
  the channel range ``c0 .. c1`` inclusive, and per source ``x_ref = x[(c0 + c1 + 1) // 2]`` and ``width
  = cube.range_width(x, c0, c1 + 1, channel_width)`` -- what :class:`cube.Moments` uses over that range.
* The ragged layout: source ``s`` owns ``h_s * w_s`` entries from ``offset_s`` on; the entry of its pixel
  ``(y, x)`` is ``offset_s + (y - y0_s) * w_s + (x - x0_s)``; ``total = offset_N + h_N * w_N <= 2^31 - 2``.
  Boxes of different sources may overlap in the plane; their entries do not.
* A voxel ``(c, p, y, x)`` with label ``s`` enters entry ``(s, y, x)`` iff ``1 <= s <= N``, ``filled[c]``,
  ``p == pol_s``, the pixel is in the source's box, ``c0_s <= c <= c1_s`` and the entry's index is below
  ``total``.  Everything else is skipped; unfilled channels are not read.
* Per entry, over the voxels that enter in ascending channel order, the sample rule of :mod:`.cube`
  without a cut: only a finite ``I`` counts; ``n += 1; d = x[c] - x_ref_s; S0 += I; t = I * d; S1 += t;
  S2 += t * d`` in float64, unfused; the peak (float32, from -inf) is replaced only if ``I > peak``.
* Outputs, float32 per entry: moment 0 = ``S0 * width_s``; 1 = ``x_ref_s + S1 / S0``; 2 =
  ``sqrt(max(0, S2 / S0 - r * r))``; 8 = the peak; 9 = x of the peak's channel; ``count`` = n (int32).  NaN
  where ``n == 0``, moments 1 and 2 also unless ``S0 > 0``: a box pixel that the source never touches
  reads NaN and count 0.
* Entry ``(s, y, x)`` equals, bit for bit and moment 2 included, what :class:`cube.Moments` gives at
  ``(pol_s, y, x)`` over ``channels=(c0_s, c1_s + 1)`` on the cube with every voxel not labelled ``s``
  blanked.  No atomics: equal inputs give equal bits.  Labels and cube are never written.

Not done: pasting the maps back into one plane; FITS cut-outs with a shifted reference pixel; a noise cut
or Hanning selection per source; sources across polarizations; cubes across several GPUs.  Why these
rules, and what the kernels cost, is DESIGN.md 5.34.
"""
import ctypes

import numpy as np

from . import accel
from ._lib import lib, check
from .channel_block import integer
from .cube import MOMENT_BITS
from .cube_operator import (AXES, SPEED_OF_LIGHT_KMS, CubeOperator, CubeTemplate, SpectralCube, _rest_frequency,
                            channel_pitch, host_filled, is_bool, velocities)
from .link import _labels

MAX_TOTAL = 2 ** 31 - 2
#: ``kimg_source_map_row`` of include/kimg.h
ROW_DTYPE = np.dtype([(name, np.int32) for name in ('offset', 'pol', 'y0', 'x0', 'h', 'w', 'c0', 'c1')]
                     + [('x_ref', np.float64), ('width', np.float64)])
_OUTPUTS = (0, 1, 2, 8, 9, 'count')
_CATALOGUE_FIELDS = ('polarization', 'c0', 'c1', 'y0', 'y1', 'x0', 'x1')


def _moments(moments):
    try:
        moments = tuple(moments)
    except TypeError:
        raise ValueError('moments must be a sequence') from None
    if not moments:
        raise ValueError('no moments asked for')
    for m in moments:
        if is_bool(m) or not isinstance(m, (int, np.integer)) or int(m) not in (0, 1, 2, 8, 9):
            raise ValueError('moments must come from 0, 1, 2, 8, 9, not {!r}'.format(m))
    moments = tuple(int(m) for m in moments)
    if len(set(moments)) != len(moments):
        raise ValueError('a moment is listed twice')
    return tuple(sorted(moments))


def _outputs(outputs):
    outputs = tuple(outputs)
    if not outputs or any(is_bool(key) or key not in _OUTPUTS for key in outputs) \
            or len(set(outputs)) != len(outputs):
        raise ValueError("outputs must be different keys from 0, 1, 2, 8, 9 and 'count'")
    return tuple(key for key in _OUTPUTS if key in outputs)


def source_rows(polarization, y0, y1, x0, x1, c0, c1, x, channel_width=None, max_entries=MAX_TOTAL):
    """``(rows, total)``: the :data:`ROW_DTYPE` table for sources whose inclusive boxes and channel
    ranges are the arguments (the catalogue's columns, [N] each), with the offsets of the ragged layout in
    the order given, and its length.  ``x`` float64 [C]: the coordinate of every channel;
    ``channel_width``, on the axis of x, serves the sources of one channel (ValueError without it).  A
    total above ``max_entries`` raises ValueError."""
    x = np.ascontiguousarray(x, np.float64)
    if x.ndim != 1 or not len(x):
        raise ValueError('x must have one entry per channel')
    columns = [np.asarray(column) for column in (polarization, y0, y1, x0, x1, c0, c1)]
    N = len(columns[0]) if columns[0].ndim == 1 else -1
    for column in columns:
        if column.shape != (N,) or (N and column.dtype.kind not in 'iu'):
            raise ValueError('polarization, y0, y1, x0, x1, c0 and c1 must be integer arrays [N]')
    pol, y0, y1, x0, x1, c0, c1 = (column.astype(np.int64) for column in columns)
    h, w = y1 - y0 + 1, x1 - x0 + 1
    if N and (min(pol.min(), y0.min(), x0.min()) < 0 or min(h.min(), w.min()) < 1
              or max(pol.max(), y1.max(), x1.max()) > 2 ** 31 - 1):
        raise ValueError('a box is empty or leaves the plane')
    if N and (c0.min() < 0 or (c1 - c0).min() < 0 or c1.max() >= len(x)):
        raise ValueError('a channel range is empty or leaves the band')
    area = h * w
    total = int(area.sum())
    if total > max_entries:
        raise ValueError('the boxes of the sources hold {} entries, more than max_entries = {}'.format(
            total, max_entries))
    rows = np.zeros(N, ROW_DTYPE)
    rows['offset'] = np.cumsum(area) - area
    for name, column in (('pol', pol), ('y0', y0), ('x0', x0), ('h', h), ('w', w), ('c0', c0), ('c1', c1)):
        rows[name] = column
    rows['x_ref'] = x[(c0 + c1 + 1) // 2]
    # cube.range_width for every source at once: the absolute mean spacing of x over c0 .. c1
    span = c1 - c0
    rows['width'] = np.abs(x[c1] - x[c0]) / np.maximum(span, 1).astype(np.float64)
    if N and span.min() == 0:
        if channel_width is None:
            raise ValueError('a range of one channel needs the channel width')
        one = abs(float(channel_width))
        if one != one:
            raise ValueError('the channel width is NaN')
        rows['width'][span == 0] = one
    return rows, total


def _rows(rows):
    rows = np.asarray(rows)
    if rows.dtype != ROW_DTYPE or rows.ndim != 1:
        raise ValueError('rows must be a ROW_DTYPE array [N]')
    return rows


def _owners(rows, total):
    """Per entry 0 .. total - 1: (the row it lies in, or 0; whether it lies in one) -- the last row whose
    offset is not above the entry, if the entry is inside that row's box."""
    at = np.arange(total, dtype=np.int64)
    if not len(rows):
        return np.zeros(total, np.int64), np.zeros(total, bool)
    offsets = rows['offset'].astype(np.int64)
    own = np.searchsorted(offsets, at, side='right') - 1
    found = own >= 0
    own = np.maximum(own, 0)
    r = rows[own]
    h, w = r['h'].astype(np.int64), r['w'].astype(np.int64)
    owned = found & (r['offset'] >= 0) & (h > 0) & (w > 0) & (at - r['offset'] < h * w)
    return own, owned


def source_maps_host(labels, cube, filled, rows, total, x, outputs=_OUTPUTS):
    """The contract of ``kimg_cube_source_maps`` and ``kimg_source_maps_finish`` in numpy: ``{key: table
    of `total` entries}`` for the keys of ``outputs`` (moments as float32, ``'count'`` as int32).
    ``labels`` int32 and ``cube`` float32 [C][P][H][W], ``filled`` [C], ``rows`` a :data:`ROW_DTYPE`
    array in ascending offset, ``x`` float64 [C].  Every sum runs in ascending channel order."""
    labels = _labels(labels)
    cube = np.asarray(cube)
    if cube.dtype != np.float32 or cube.shape != labels.shape:
        raise ValueError('cube must be float32 of the shape of labels')
    C, P, H, W = labels.shape
    filled = host_filled(filled, C)
    rows = _rows(rows)
    x = np.ascontiguousarray(x, np.float64)
    if x.shape != (C,):
        raise ValueError('x must have one entry per channel')
    total = int(total)
    if total < 0:
        raise ValueError('a negative total')
    outputs = _outputs(outputs)
    N = len(rows)
    member = (labels > 0) & (labels <= N) & filled.reshape(-1, 1, 1, 1)
    d = np.flatnonzero(member.reshape(-1))              # ascending dense index: ascending channel
    r = rows[labels.reshape(-1)[d].astype(np.int64) - 1]
    c = d // (P * H * W)
    dy = d % (H * W) // W - r['y0'].astype(np.int64)
    dx = d % W - r['x0'].astype(np.int64)
    at = r['offset'].astype(np.int64) + dy * r['w'].astype(np.int64) + dx
    enters = ((d % (P * H * W) // (H * W) == r['pol']) & (dy >= 0) & (dy < r['h']) & (dx >= 0) & (dx < r['w'])
              & (r['offset'] >= 0) & (at < total) & (c >= r['c0']) & (c <= r['c1']))
    f = cube.reshape(-1)[d]
    enters &= np.isfinite(f)
    at, c, f, x_ref = at[enters], c[enters], f[enters], r['x_ref'][enters]
    Id = f.astype(np.float64)
    n = np.bincount(at, minlength=total).astype(np.int32)
    S0, S1, S2 = np.zeros(total), np.zeros(total), np.zeros(total)
    with np.errstate(all='ignore'):
        dd = x[c] - x_ref
        t = Id * dd
        np.add.at(S0, at, Id)                           # (unbuffered: one by one, in the order given)
        np.add.at(S1, at, t)
        np.add.at(S2, at, t * dd)
    # the peak is replaced only by a larger value: the first voxel that holds the entry's maximum
    top = np.full(total, -np.inf, np.float32)
    np.maximum.at(top, at, f)
    holds = np.flatnonzero(f == top[at])
    entries, first = np.unique(at[holds], return_index=True)
    peak = np.full(total, -np.inf, np.float32)
    peak_channel = np.zeros(total, np.int64)
    peak[entries] = f[holds[first]]
    peak_channel[entries] = c[holds[first]]

    own, owned = _owners(rows, total)
    n = np.where(owned, n, 0).astype(np.int32)
    width = rows['width'][own] if N else np.zeros(total)
    x_ref = rows['x_ref'][own] if N else np.zeros(total)
    nan = np.full(total, np.nan, np.float32)
    with np.errstate(all='ignore'):
        some = n > 0
        positive = some & (S0 > 0)
        ratio = S1 / S0
        v = S2 / S0 - ratio * ratio
        v = np.where(v < 0, 0.0, v)
        values = {
            0: np.where(some, (S0 * width).astype(np.float32), nan),
            1: np.where(positive, (x_ref + ratio).astype(np.float32), nan),
            2: np.where(positive, np.sqrt(v).astype(np.float32), nan),
            8: np.where(some, peak, nan),
            9: np.where(some, x[peak_channel].astype(np.float32), nan),
            'count': n,
        }
    return {key: np.ascontiguousarray(values[key], np.int32 if key == 'count' else np.float32)
            for key in outputs}


class SourceMapParameters:
    """``moments``: a subset of {0, 1, 2, 8, 9}, as in :class:`cube.MomentParameters`.  ``axis``:
    'velocity' (radio convention, km/s, needs ``rest_frequency`` in Hz) or 'frequency' (Hz).
    ``max_entries``: the largest sum of box areas a call may be asked for; every entry costs 36 bytes of
    state and 4 bytes per output table on the device."""

    def __init__(self, moments=(0, 1, 2), axis='velocity', rest_frequency=None, max_entries=2 ** 26):
        self.moments = _moments(moments)
        if axis not in AXES:
            raise ValueError("axis must be 'velocity' or 'frequency'")
        self.axis = axis
        if rest_frequency is not None:
            if is_bool(rest_frequency):
                raise ValueError('rest_frequency must be a number, not a bool')
            rest_frequency = _rest_frequency(rest_frequency)
        self.rest_frequency = rest_frequency
        if self.axis == 'velocity' and self.rest_frequency is None:
            raise ValueError('the velocity axis needs a rest frequency')
        if is_bool(max_entries):
            raise ValueError('max_entries must be an integer, not a bool')
        self.max_entries = integer(max_entries, 'max_entries', 1, MAX_TOTAL)

    def __repr__(self):
        return 'SourceMapParameters({!r}, axis={!r}, rest_frequency={!r}, max_entries={!r})'.format(
            self.moments, self.axis, self.rest_frequency, self.max_entries)


class SourceMaps:
    """The ragged maps of one :class:`SourceMapper` call.  ``tables``: ``{moment: device float32
    [total], 'count': device int32 [total]}``; ``rows`` (host :data:`ROW_DTYPE` [N]) holds the boxes and
    ``offsets`` (host int64 [N + 1]) says which entries are whose.  ``ready`` fires when the call has
    written the tables; :meth:`get` makes its queue wait for that on the device first."""

    def __init__(self, rows, total, keys, tables, ready, command_queue):
        self.rows = rows
        self.total = total
        self.offsets = np.append(rows['offset'].astype(np.int64), total)
        self.keys = keys
        self.tables = tables
        self.ready = ready
        self.command_queue = command_queue
        self._host = None

    def __len__(self):
        return len(self.rows)

    def get(self, command_queue=None):
        """``{key: host table of `total` entries}``."""
        if self._host is None:
            queue = self.command_queue if command_queue is None else command_queue
            if self.total == 0:
                self._host = {key: np.zeros(0, np.int32 if key == 'count' else np.float32) for key in self.keys}
            else:
                if self.ready is not None:
                    queue.enqueue_wait_for_events([self.ready])
                self._host = {key: table.get(queue) for key, table in self.tables.items()}
        return self._host

    def _source(self, source):
        if is_bool(source) or not isinstance(source, (int, np.integer)) or not 1 <= source <= len(self):
            raise ValueError('source must be 1 to {}'.format(len(self)))
        return self.rows[int(source) - 1]

    def map(self, source, command_queue=None):
        """``{moment: float32 [h][w], 'count': int32 [h][w]}`` of source ``source`` (1 to N)."""
        row = self._source(source)
        a = int(row['offset'])
        shape = (int(row['h']), int(row['w']))
        return {key: table[a:a + shape[0] * shape[1]].reshape(shape).copy()
                for key, table in self.get(command_queue).items()}

    def origin(self, source):
        """``(polarization, y0, x0)`` of the map of source ``source``."""
        row = self._source(source)
        return int(row['pol']), int(row['y0']), int(row['x0'])


class SourceMapper(CubeOperator):
    """The per-source moment maps for cubes of shape ``cube_shape`` = (C, P, H, W).  ``op(labels,
    the_cube, catalogue)`` takes a :class:`link.LabelCube`, a :class:`cube.SpectralCube` and the catalogue
    of :class:`link.Link` (its ``polarization, c0, c1, y0, y1, x0, x1`` are read); ``op(labels, array,
    catalogue, filled=..., frequencies=...)`` takes a plain float32 :class:`accel.DeviceArray` whose
    [P][H][W] plane is dense, with ``channel_width`` (Hz) for sources of a single channel.  It returns a
    :class:`SourceMaps`.

    A call makes the rows on the host, uploads them with the coordinates in one copy (48 bytes a source),
    allocates the state and the output tables, waits on the device for the labels' ``ready`` and enqueues
    a memset and two kernels on ``command_queue``; the host waits for nothing.  An empty catalogue returns
    an empty result without a launch; a sum of box areas above ``max_entries`` raises ValueError."""

    def __init__(self, template, command_queue, cube_shape):
        super().__init__(template, command_queue, cube_shape, band=True)
        C, P, H, W = self.cube_shape
        if C * P * H * W > 2 ** 31 - 2:
            raise ValueError('more than 2^31 - 2 voxels: labels are int32')

    def _coordinates(self, cube, frequencies, channel_width):
        """(x, the channel width on its axis or None)"""
        params = self.params
        if isinstance(cube, SpectralCube):
            return (cube.coordinates(params.axis, params.rest_frequency),
                    cube.axis_channel_width(params.axis, params.rest_frequency))
        if frequencies is None:
            raise ValueError('a plain array needs frequencies')
        frequencies = np.asarray(frequencies, np.float64)
        if frequencies.shape != (self.cube_shape[0],):
            raise ValueError('frequencies must have one entry per channel')
        if channel_width is not None:
            channel_width = abs(float(channel_width))
        if params.axis == 'frequency':
            return frequencies.copy(), channel_width
        if channel_width is not None:
            channel_width = channel_width / params.rest_frequency * SPEED_OF_LIGHT_KMS
        return velocities(frequencies, params.rest_frequency), channel_width

    def __call__(self, labels, cube, catalogue, filled=None, frequencies=None, channel_width=None):
        params = self.params
        C, P, H, W = self.cube_shape
        queue = self.command_queue
        labels, array = self._arrays((labels, 'labels', np.int32), (cube, 'cube', np.float32))
        filled = self._filled(self._own_filled(cube, filled, frequencies=frequencies,
                                               channel_width=channel_width))
        x, channel_width = self._coordinates(cube, frequencies, channel_width)
        catalogue = np.asarray(catalogue)
        if catalogue.ndim != 1 or catalogue.dtype.names is None \
                or not set(_CATALOGUE_FIELDS) <= set(catalogue.dtype.names):
            raise ValueError('catalogue must be a structured array with ' + ', '.join(_CATALOGUE_FIELDS))
        N = len(catalogue)
        if N and (int(catalogue['polarization'].max()) >= P or int(catalogue['y1'].max()) >= H
                  or int(catalogue['x1'].max()) >= W or int(catalogue['c1'].max()) >= C):
            raise ValueError('a source of the catalogue leaves the cube')
        rows, total = source_rows(*(catalogue[name] for name in ('polarization', 'y0', 'y1', 'x0', 'x1', 'c0', 'c1')),
                                  x, channel_width, params.max_entries)
        keys = params.moments + ('count',)
        if N == 0:
            return SourceMaps(rows, 0, keys, {}, None, queue)
        pitch = channel_pitch(array)
        label_pitch = channel_pitch(labels)
        self._wait_ready(labels)
        labels.used_on(queue)
        array.used_on(queue)
        context = queue.context
        # [x (C float64)][rows (N of 48 bytes)] in one array, one upload
        tables = accel.DeviceArray(context, (8 * C + ROW_DTYPE.itemsize * N,), np.uint8, queue=queue)
        tables.set_async(queue, np.concatenate((np.ascontiguousarray(x, np.float64).view(np.uint8),
                                                rows.view(np.uint8))))
        x_ptr, rows_ptr = tables.ptr, tables.ptr + 8 * C
        state_bytes = lib().kimg_cube_source_maps_workspace_bytes(total)
        state = accel.DeviceArray(context, (state_bytes // 8 + 1,), np.float64, queue=queue)
        out = {key: accel.DeviceArray(context, (total,), np.int32 if key == 'count' else np.float32, queue=queue)
               for key in keys}
        outputs = 0
        for key in keys:
            outputs |= MOMENT_BITS[key]
        handle = queue.handle
        check(lib().kimg_cube_source_maps(
            labels.ptr, label_pitch, array.ptr, pitch, C, P, H, W, filled.ctypes.data_as(ctypes.c_void_p),
            x_ptr, N, rows_ptr, total, state.ptr, state_bytes, handle), 'kimg_cube_source_maps')
        pointers = [out[key].ptr if key in out else None for key in _OUTPUTS]
        check(lib().kimg_source_maps_finish(N, rows_ptr, total, state.ptr, state_bytes, x_ptr, C, outputs,
                                            *pointers, handle), 'kimg_source_maps_finish')
        return SourceMaps(rows, total, keys, out, queue.enqueue_marker(), queue)


class SourceMapsTemplate(CubeTemplate):
    params_type = SourceMapParameters
    operator = SourceMapper
