"""Source linking: :mod:`.detect`'s mask is a cloud of set voxels; a source finder ends with sources --
which voxels belong together, how many sources there are, where each one is, how bright it is and
which are too small to be real (SoFiA's linker and parameteriser, the seeds of CASA's ``imfit``, the
region list ``immoments`` takes per source).

:class:`LinkTemplate` / :class:`Link` is the linker on the device (csrc/cube_link.hip:
``kimg_cube_link``, ``kimg_cube_measure``, ``kimg_cube_link_filter``), on one queue with a single wait
at the end, for the catalogue.  ``op(mask, the_cube)`` returns ``(labels, catalogue)``: a
:class:`LabelCube`, device int32 [C][P][H][W], whose :meth:`LabelCube.mask` (``kimg_cube_label_mask``)
gives the :class:`detect.MaskCube` of all kept sources or of one, and a numpy structured array with a
row per source.  :func:`link_host`, :func:`measure_host`, :func:`filter_host` and
:func:`label_mask_host` are the contracts as numpy: the executable specification.

The contracts (include/kimg.h, "Source linking").  A voxel is set iff its channel is filled and its
mask byte is nonzero.  ``d = ((c * P + p) * H + y) * W + x`` is its dense index.

* ``link``: set voxels (c, p, y, x) and (c', p', y', x') are neighbours iff ``p == p'``,
  ``|c - c'| <= reach_z`` (0 to 3; it counts channels, filled or not) and
  ``(x - x')^2 + (y - y')^2 <= reach_xy_sq`` (0 to 9).  A source is a connected component.  Labels are 0
  where not set and else the source's number, 1 to N0, sources numbered in ascending order of their
  smallest dense index.  At ``reach_xy_sq`` 1 or 2 and ``reach_z <= 1`` that is
  ``scipy.ndimage.label`` with a structure that is empty along P.
* ``measure``: per source over its voxels (filled channels): ``first`` (smallest dense index),
  ``voxels``, ``finite`` (those with a finite cube value), the inclusive box; over the finite ones the
  ``peak`` -- largest in ``kimg_cube_stats``' order, -0 below +0, smallest dense index on ties -- and
  the ``trough`` likewise, NaN and -1 without any; ``sum = sum f``, ``sum_c = sum f * c``, ``sum_y``,
  ``sum_x`` in float64, one product per term.  The twin sums in ascending dense index; the device's
  order is not fixed (float64 atomics), so the sums agree exactly where every order gives the exact
  sum and to ``n * 2^-53 * sum |term|`` otherwise.
* ``filter``: a source is kept iff ``voxels >= min_voxels``, both plane extents ``>= min_size_xy`` and
  the channel extent ``>= min_size_z``; kept sources are renumbered 1 to N in their old order.
* ``label_mask``: 1 where the label is nonzero (``source == 0``) or equals ``source``, 0 elsewhere.

Python's ``radius_xy`` (0 to 3) becomes ``reach_xy_sq = floor(radius_xy^2)``: 1 is 4-connectivity in
the plane (SoFiA's default), 1.5 is 8-connectivity, 2 and 3 bridge gaps.

Why these rules, and what the kernels cost, is DESIGN.md 5.31.

Per-source spectra, fluxes in Jy with their errors and line widths are :mod:`.sources`'; the moment maps
of every source inside its own box are :mod:`.source_maps`'.

Not done: reliability from negative detections; mask dilation; sources across polarizations; cubes
across several GPUs; bit-reproducible sums.
"""
import ctypes
import math

import numpy as np

from . import accel
from ._lib import lib, check, Catalogue
from .channel_block import integer
from .cube_operator import (CubeOperator, CubeTemplate, ReadyArray, SpectralCube, band_size, channel_pitch,
                            host_filled, is_bool, wait_ready)
from .detect import MaskCube

MAX_REACH_XY_SQ = 9
MAX_REACH_Z = 3

_INT_FIELDS = ('first', 'voxels', 'finite', 'c0', 'c1', 'y0', 'y1', 'x0', 'x1', 'peak_index',
               'trough_index')
_FLOAT_FIELDS = ('peak', 'trough')
_SUM_FIELDS = ('sum', 'sum_c', 'sum_y', 'sum_x')
#: what ``measure_host`` returns and ``kimg_cube_measure`` fills, a row per source
TABLE_DTYPE = np.dtype([(name, np.int32) for name in _INT_FIELDS]
                       + [(name, np.float32) for name in _FLOAT_FIELDS]
                       + [(name, np.float64) for name in _SUM_FIELDS])
#: a row of the catalogue that the operator returns
CATALOGUE_DTYPE = np.dtype(
    [('id', np.int32), ('polarization', np.int32), ('voxels', np.int32), ('finite', np.int32)]
    + [(name, np.int32) for name in ('c0', 'c1', 'y0', 'y1', 'x0', 'x1')]
    + [('peak', np.float32), ('peak_c', np.int32), ('peak_y', np.int32), ('peak_x', np.int32),
       ('trough', np.float32), ('trough_c', np.int32), ('trough_y', np.int32), ('trough_x', np.int32),
       ('sum', np.float64), ('centroid', np.float64, (3,)), ('frequency', np.float64)])

_QUIET = np.array([0x7fc00000], np.uint32).view(np.float32)[0]


class TooManySources(RuntimeError):
    """The mask links into ``count`` sources, more than ``max_sources``.  ``labels`` is the
    :class:`LabelCube` of all of them, 1 to ``count``, unfiltered."""

    def __init__(self, count, max_sources, labels=None):
        super().__init__('{} sources, max_sources is {}'.format(count, max_sources))
        self.count = count
        self.max_sources = max_sources
        self.labels = labels


def _reach(reach_xy_sq, reach_z):
    if is_bool(reach_xy_sq) or is_bool(reach_z):
        raise ValueError('a reach must be an integer, not a bool')
    return (integer(reach_xy_sq, 'reach_xy_sq', 0, MAX_REACH_XY_SQ),
            integer(reach_z, 'reach_z', 0, MAX_REACH_Z))


def _set_voxels(mask, filled):
    mask = np.asarray(mask)
    if mask.dtype != np.uint8 and mask.dtype != np.bool_:
        raise TypeError('mask must be uint8 or bool')
    if mask.ndim != 4:
        raise ValueError('mask must be [channel][polarization][y][x]')
    band_size(mask.shape[0])
    if mask.size > 2 ** 31 - 2:
        raise ValueError('more than 2^31 - 2 voxels')
    return (mask != 0) & host_filled(filled, mask.shape[0]).reshape(-1, 1, 1, 1)


def neighbour_offsets(reach_xy_sq, reach_z):
    """The (dz, dy, dx) that lead from a voxel to its neighbours of SMALLER dense index."""
    reach_xy_sq, reach_z = _reach(reach_xy_sq, reach_z)
    radius = math.isqrt(reach_xy_sq)
    return [(dz, dy, dx)
            for dz in range(-reach_z, 1) for dy in range(-radius, radius + 1)
            for dx in range(-radius, radius + 1)
            if dx * dx + dy * dy <= reach_xy_sq and (dz, dy, dx) < (0, 0, 0)]


def link_host(mask, filled, reach_xy_sq=1, reach_z=1):
    """The contract of ``kimg_cube_link`` in numpy.  ``mask`` uint8 or bool [C][P][H][W], ``filled``
    [C].  Returns ``(labels, N0)``, labels int32 of the mask's shape."""
    on = _set_voxels(mask, filled)
    offsets = neighbour_offsets(reach_xy_sq, reach_z)
    C, P, H, W = on.shape
    # the set voxels in ascending dense index are 0 .. n - 1; ident: a voxel's place among them
    ident = np.full(on.shape, -1, np.int64)
    n = int(on.sum())
    ident[on] = np.arange(n)
    a, b = [], []
    for dz, dy, dx in offsets:
        if -dz >= C or abs(dy) >= H or abs(dx) >= W:
            continue
        here = (slice(-dz, C), slice(None), slice(max(-dy, 0), H - max(dy, 0)),
                slice(max(-dx, 0), W - max(dx, 0)))
        there = (slice(0, C + dz), slice(None), slice(max(dy, 0), H - max(-dy, 0)),
                 slice(max(dx, 0), W - max(-dx, 0)))
        both = on[here] & on[there]
        a.append(ident[here][both])
        b.append(ident[there][both])
    a = np.concatenate(a) if a else np.zeros(0, np.int64)
    b = np.concatenate(b) if b else np.zeros(0, np.int64)
    # hook the larger root under the smaller, then make every voxel point at its root; repeat
    parent = np.arange(n)
    while True:
        pa, pb = parent[a], parent[b]
        differ = pa != pb
        if not differ.any():
            break
        np.minimum.at(parent, np.maximum(pa, pb)[differ], np.minimum(pa, pb)[differ])
        while True:
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up
    roots, number = np.unique(parent, return_inverse=True)
    labels = np.zeros(on.shape, np.int32)
    labels[on] = number.reshape(-1) + 1
    return labels, len(roots)


def _labels(labels):
    labels = np.asarray(labels)
    if labels.dtype != np.int32 or labels.ndim != 4:
        raise ValueError('labels must be int32 [channel][polarization][y][x]')
    return labels


def value_keys(values):
    """``kimg_cube_stats``' order of float32 values as uint32: -0 lies below +0."""
    bits = np.ascontiguousarray(values, np.float32).view(np.uint32)
    return bits ^ np.where(bits >> 31, np.uint32(0xffffffff), np.uint32(0x80000000))


def measure_host(labels, cube, filled, num_sources=None, capacity=None):
    """The contract of ``kimg_cube_measure`` in numpy: a :data:`TABLE_DTYPE` array with a row for each
    of the sources 1 to ``min(num_sources, capacity)`` (``num_sources`` None: the largest label).  The
    sums run in ascending dense index."""
    labels = _labels(labels)
    cube = np.asarray(cube)
    if cube.dtype != np.float32 or cube.shape != labels.shape:
        raise ValueError('cube must be float32 of the shape of labels')
    C, P, H, W = labels.shape
    member = (labels > 0) & host_filled(filled, C).reshape(-1, 1, 1, 1)
    if num_sources is None:
        num_sources = int(labels[member].max()) if member.any() else 0
    rows = num_sources if capacity is None else min(num_sources, capacity)
    member &= labels <= rows
    d = np.flatnonzero(member.reshape(-1))              # ascending dense index
    s = labels.reshape(-1)[d].astype(np.int64) - 1
    f = cube.reshape(-1)[d]
    c, rest = np.divmod(d, P * H * W)
    y, x = np.divmod(rest % (H * W), W)
    table = np.zeros(rows, TABLE_DTYPE)
    table['voxels'] = np.bincount(s, minlength=rows)
    big = np.iinfo(np.int64).max
    for name, value, low in (('first', d, True), ('c0', c, True), ('c1', c, False), ('y0', y, True),
                             ('y1', y, False), ('x0', x, True), ('x1', x, False)):
        out = np.full(rows, big if low else -1, np.int64)
        (np.minimum if low else np.maximum).at(out, s, value)
        table[name] = np.where(table['voxels'] > 0, out, 0)
    ok = np.isfinite(f)
    d, s, f, c, y, x = d[ok], s[ok], f[ok], c[ok], y[ok], x[ok]
    table['finite'] = np.bincount(s, minlength=rows)
    t = f.astype(np.float64)
    for name, term in (('sum', t), ('sum_c', t * c.astype(np.float64)), ('sum_y', t * y.astype(np.float64)),
                       ('sum_x', t * x.astype(np.float64))):
        out = np.zeros(rows, np.float64)
        np.add.at(out, s, term)                         # (unbuffered: one by one, in the order given)
        table[name] = out
    keys = value_keys(f).astype(np.int64)
    table['peak'] = table['trough'] = _QUIET
    table['peak_index'] = table['trough_index'] = -1
    for name, order in (('peak', np.lexsort((d, -keys, s))), ('trough', np.lexsort((d, keys, s)))):
        # the first voxel of every source in (key, then dense index) order
        heads = order[np.r_[True, np.diff(s[order]) != 0]] if len(order) else order
        table[name][s[heads]] = f[heads]
        table[name + '_index'][s[heads]] = d[heads]
    return table


def _minimum(value, name):
    if is_bool(value):
        raise ValueError('{} must be an integer, not a bool'.format(name))
    return integer(value, name, 1, 2 ** 31 - 1)


def filter_host(labels, table, min_voxels=1, min_size_xy=1, min_size_z=1):
    """The contract of ``kimg_cube_link_filter`` in numpy, for a table with a row for every source.
    Returns ``(labels, table)``, new arrays."""
    labels = _labels(labels)
    table = np.asarray(table)
    if table.dtype != TABLE_DTYPE or table.ndim != 1:
        raise ValueError('table must be what measure_host returns')
    min_voxels = _minimum(min_voxels, 'min_voxels')
    min_size_xy = _minimum(min_size_xy, 'min_size_xy')
    min_size_z = _minimum(min_size_z, 'min_size_z')
    if labels.size and labels.max() > len(table):
        raise ValueError('a label without a row')
    keep = ((table['voxels'] >= min_voxels) & (table['x1'] - table['x0'] + 1 >= min_size_xy)
            & (table['y1'] - table['y0'] + 1 >= min_size_xy) & (table['c1'] - table['c0'] + 1 >= min_size_z))
    number = np.zeros(len(table) + 1, np.int32)
    number[1:] = np.where(keep, np.cumsum(keep), 0)
    return number[np.maximum(labels, 0)], table[keep].copy()


def label_mask_host(labels, source=0):
    """The contract of ``kimg_cube_label_mask`` in numpy: uint8 of the labels' shape."""
    labels = _labels(labels)
    if is_bool(source):
        raise ValueError('source must be an integer, not a bool')
    source = integer(source, 'source', 0, 2 ** 31 - 1)
    return (labels == source if source else labels != 0).astype(np.uint8)


def catalogue_host(table, shape, frequencies=None):
    """The :data:`CATALOGUE_DTYPE` rows of a measured table for cubes of ``shape`` = (C, P, H, W): ids 1
    to N, the polarization, the peak's and trough's (c, y, x), the centroid ``(sum_c, sum_y, sum_x) /
    sum`` in float64 (NaN where ``sum == 0``) and the frequency at the centroid channel, interpolated
    linearly between the channels' ``frequencies`` (NaN without them or without a centroid)."""
    C, P, H, W = shape
    table = np.asarray(table)
    out = np.zeros(len(table), CATALOGUE_DTYPE)
    out['id'] = np.arange(1, len(table) + 1)
    out['polarization'] = table['first'] % (P * H * W) // (H * W)
    for name in ('voxels', 'finite', 'c0', 'c1', 'y0', 'y1', 'x0', 'x1', 'peak', 'trough', 'sum'):
        out[name] = table[name]
    for name in ('peak', 'trough'):
        index = table[name + '_index'].astype(np.int64)
        none = index < 0
        out[name + '_c'] = np.where(none, -1, index // (P * H * W))
        out[name + '_y'] = np.where(none, -1, index % (H * W) // W)
        out[name + '_x'] = np.where(none, -1, index % W)
    with np.errstate(divide='ignore', invalid='ignore'):
        for k, name in enumerate(('sum_c', 'sum_y', 'sum_x')):
            out['centroid'][:, k] = np.where(table['sum'] == 0, np.nan, table[name] / table['sum'])
    out['frequency'] = np.nan
    if frequencies is not None:
        frequencies = np.asarray(frequencies, np.float64)
        at = out['centroid'][:, 0]
        inside = np.isfinite(at) & (at >= 0) & (at <= C - 1)
        out['frequency'][inside] = np.interp(at[inside], np.arange(C), frequencies)
    return out


class LinkParameters:
    """``radius_xy`` (0 to 3, a float) and ``radius_z`` (0 to 3 channels, an integer): how far apart
    two set voxels of one polarization may be and still belong together -- 1 is 4-connectivity in the
    plane, 1.5 is 8-connectivity, 2 and 3 bridge gaps.  ``min_voxels``, ``min_size_xy``, ``min_size_z``:
    sources with fewer voxels, or a bounding box narrower in x or y or shorter along the channels, are
    dropped.  ``max_sources``: the rows of the device catalogue; a mask with more sources raises
    :class:`TooManySources`."""

    def __init__(self, radius_xy=1, radius_z=1, min_voxels=1, min_size_xy=1, min_size_z=1,
                 max_sources=65536):
        if is_bool(radius_xy):
            raise ValueError('radius_xy must be a number, not a bool')
        try:
            radius_xy = float(radius_xy)
        except (TypeError, ValueError):
            raise ValueError('radius_xy must be a number') from None
        if not 0.0 <= radius_xy <= 3.0:                 # (false for NaN)
            raise ValueError('radius_xy must be 0 to 3')
        if is_bool(radius_z):
            raise ValueError('radius_z must be an integer, not a bool')
        self.radius_xy = radius_xy
        self.radius_z = integer(radius_z, 'radius_z', 0, MAX_REACH_Z)
        self.reach_xy_sq = int(math.floor(radius_xy * radius_xy))
        self.min_voxels = _minimum(min_voxels, 'min_voxels')
        self.min_size_xy = _minimum(min_size_xy, 'min_size_xy')
        self.min_size_z = _minimum(min_size_z, 'min_size_z')
        if is_bool(max_sources):
            raise ValueError('max_sources must be an integer, not a bool')
        self.max_sources = integer(max_sources, 'max_sources', 1, 2 ** 24)

    @property
    def filters(self):
        return self.min_voxels > 1 or self.min_size_xy > 1 or self.min_size_z > 1

    def __repr__(self):
        return ('LinkParameters(radius_xy={!r}, radius_z={!r}, min_voxels={!r}, min_size_xy={!r}, '
                'min_size_z={!r}, max_sources={!r})').format(
                    self.radius_xy, self.radius_z, self.min_voxels, self.min_size_xy, self.min_size_z,
                    self.max_sources)


class LabelCube(ReadyArray):
    """Source labels, device int32 [C][P][H][W]: 0 = no source, s = source s of the catalogue; a
    :class:`cube_operator.ReadyArray`, whose ``filled`` (uint8 [C]) is what the linker was told."""

    def mask(self, source=0):
        """``kimg_cube_label_mask``: the :class:`detect.MaskCube` of every source (``source`` 0) or of
        source ``source`` alone, on the labels' queue."""
        if is_bool(source):
            raise ValueError('source must be an integer, not a bool')
        source = integer(source, 'source', 0, 2 ** 31 - 1)
        queue = self.command_queue
        wait_ready(queue, self)
        self.used_on(queue)
        mask = MaskCube.of_cube(queue, self.shape, np.uint8, self.filled)
        M =int(np.prod(self.shape[1:]))
        check(lib().kimg_cube_label_mask(self.ptr, M, mask.ptr, M, self.shape[0], M, source,
                                         queue.handle), 'kimg_cube_label_mask')
        mask.ready = queue.enqueue_marker()
        return mask


class Link(CubeOperator):
    """The linker for cubes of shape ``cube_shape`` = (C, P, H, W).  ``op(mask, the_cube)`` takes a
    :class:`detect.MaskCube` and a :class:`cube.SpectralCube`; ``op(mask, array, filled=...,
    frequencies=None)`` takes plain :class:`accel.DeviceArray` s (uint8 and float32) whose [P][H][W]
    plane is dense while the channel axis may have any pitch.  It returns ``(labels, catalogue)``: a
    :class:`LabelCube` and a :data:`CATALOGUE_DTYPE` array of the N kept sources.

    The operator owns the workspace and the device tables (``max_sources`` rows), allocated at
    ``instantiate``; a call allocates the labels, is a fixed sequence of launches on ``command_queue``
    and waits for the device once, at the end, when it reads the tables and the two counts."""

    def __init__(self, template, command_queue, cube_shape):
        super().__init__(template, command_queue, cube_shape, band=True)
        params = self.params
        queue = command_queue
        C, P, H, W = self.cube_shape
        if C * P * H * W > 2 ** 31 - 2:
            raise ValueError('more than 2^31 - 2 voxels: labels are int32')
        context = queue.context
        rows = params.max_sources
        words = lib().kimg_cube_link_scratch_bytes(C, P * H * W) // 4
        self._scratch = accel.DeviceArray(context, (words,), np.int32, queue=queue)
        self._work = accel.DeviceArray(context, (lib().kimg_cube_catalogue_work_bytes(rows) // 8,),
                                       np.int64, queue=queue)
        # one buffer, so that one read brings everything: [counts (2 int32, 8 more bytes unused)]
        # [the float64 sums][the int32 fields][the float32 fields], each [rows]
        self._layout = {}
        at = 16
        for names, size in ((_SUM_FIELDS, 8), (_INT_FIELDS + _FLOAT_FIELDS, 4)):
            for name in names:
                self._layout[name] = at
                at += size * rows
        self._tables = accel.DeviceArray(context, (at,), np.uint8, queue=queue)
        base = self._tables.ptr
        self._catalogue = Catalogue(work=self._work.ptr,
                                    **{name: base + at for name, at in self._layout.items()})

    def __call__(self, mask, cube, filled=None, frequencies=None):
        params = self.params
        C, P, H, W = self.cube_shape
        M = P * H * W
        queue = self.command_queue
        mask, array = self._arrays((mask, 'mask', np.uint8), (cube, 'cube', np.float32))
        filled = self._filled(self._own_filled(cube, filled, frequencies=frequencies))
        if isinstance(cube, SpectralCube):
            frequencies = cube.frequencies
        if frequencies is not None and np.shape(frequencies) != (C,):
            raise ValueError('frequencies must have one entry per channel')
        pitch = channel_pitch(array)
        mask_pitch = channel_pitch(mask)
        self._wait_ready(mask)
        mask.used_on(queue)
        array.used_on(queue)
        labels = LabelCube.of_cube(queue, self.cube_shape, np.int32, filled)
        handle = queue.handle
        filled_ptr = filled.ctypes.data_as(ctypes.c_void_p)
        counts = self._tables.ptr
        catalogue = ctypes.byref(self._catalogue)
        rows = params.max_sources
        check(lib().kimg_cube_link(mask.ptr, mask_pitch, labels.ptr, M, C, P, H, W, filled_ptr,
                                   params.reach_xy_sq, params.radius_z, self._scratch.ptr, counts, handle),
              'kimg_cube_link')
        check(lib().kimg_cube_measure(labels.ptr, M, array.ptr, pitch, C, P, H, W, filled_ptr, catalogue,
                                      rows, counts, handle), 'kimg_cube_measure')
        if params.filters:
            check(lib().kimg_cube_link_filter(labels.ptr, M, C, M, catalogue, rows, params.min_voxels,
                                              params.min_size_xy, params.min_size_z, counts, handle),
                  'kimg_cube_link_filter')
        labels.ready = queue.enqueue_marker()
        raw = self._tables.get(queue)               # (the call's only wait)
        linked, kept = (int(v) for v in raw[:8].view(np.int32))
        if linked > rows:
            raise TooManySources(linked, rows, labels)
        N = kept if params.filters else linked
        table = np.zeros(N, TABLE_DTYPE)
        for name, at in self._layout.items():
            dtype = TABLE_DTYPE[name]
            table[name] = raw[at:at + dtype.itemsize * N].view(dtype)
        return labels, catalogue_host(table, self.cube_shape, frequencies)


class LinkTemplate(CubeTemplate):
    params_type = LinkParameters
    operator = Link
