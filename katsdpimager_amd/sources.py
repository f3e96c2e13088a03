"""Source parameters: what a source finder hands back for every source that :mod:`.link` has found
(SoFiA's parameteriser) -- the integrated spectrum, the flux in Jy times the axis unit with its error,
the peak flux density, the centroid on the spectral axis and the line widths at 50 % and 20 % of the
peak.

:class:`SourcesTemplate` / :class:`Sources` is the operator on the device (csrc/cube_sources.hip:
``kimg_cube_source_spectra``, ``kimg_source_lines``).  ``op(labels, the_cube, catalogue)`` takes the
:class:`link.LabelCube` and the catalogue of one :class:`link.Link` call and returns ``(spectra,
lines)``: a :class:`SourceSpectra` -- the ragged device tables with one entry per (source, channel of
its box) -- and a numpy structured array :data:`LINES_DTYPE` with a row per source.  One pass over
labels and cube, whatever the number of sources, where ``labels.mask(source=k)``,
:meth:`detect.MaskCube.apply` and :class:`cube.Moments` are three passes per source.
:func:`source_spectra_host` and :func:`source_lines_host` are the contracts as numpy: the executable
specification.  :func:`line_tables` makes the four per-channel tables the lines need from a
:class:`cube.SpectralCube`.

The contracts (include/kimg.h, "Source spectra and line parameters").

* The ragged layout: source ``s`` (1 to N) owns the entries ``offsets[s-1] .. offsets[s] - 1``, one per
  channel ``c0[s-1] + k``; ``total = offsets[N]``.  The operator takes ``c0`` and ``c1`` of the catalogue.
* ``spectra``: per entry, over the voxels of its channel (filled) with the source's label: ``voxels``,
  ``finite`` (those with a finite cube value) and ``sum``, the float64 sum of the finite values.  Entries
  of unfilled channels read 0.  Labels outside 1 to N and channels outside a row's range are skipped.
  The counts are exact; the order of ``sum`` is not fixed on the device (float64 atomics of partial
  sums), so it equals the twin's where every order is exact and lies within ``finite * 2^-53 *
  sum |term|`` of the exactly rounded sum otherwise.
* ``lines``: with ``d_k = sum_k * unit[c]``, in float64 and ascending channel order: ``flux = sum d_k *
  width[c]``; ``flux_err = sqrt(sum finite_k * variance[c])``; ``peak`` the largest ``d_k`` over entries
  with a finite voxel and ``peak_channel`` its channel (the lowest of a tie), NaN and -1 without one;
  ``centroid = sum d_k * coord[c] / sum d_k`` (NaN where the denominator is 0); ``w50``, ``w20`` by SoFiA's
  rule -- from either end the first channel at or above half (a fifth of) the peak, the edge
  interpolated linearly between it and the channel before -- with the four edges, NaN unless
  ``peak > 0``; ``channels = n``.  Given the same spectra the device has the twin's bits.

Units (:func:`line_tables`).  A cube in Jy/beam summed over pixels is a flux density in Jy once divided
by the beam area in pixels, ``Omega = 2 pi sqrt(det Sigma)`` (``smooth.beam_covariance``): ``unit = 1 /
Omega``, of ``common_beam`` if the cube has one, else of every channel's own.  ``width`` is the channel
width on the axis.  ``variance[c] = Omega * (noise[c] * unit[c] * width[c])^2`` is what one voxel adds
to the variance of the flux: pixels within a beam are correlated, so n of them carry the noise of
``n / Omega`` independent ones, each ``Omega`` pixels' worth.

The moment maps of every source inside its own box, whose sums are bit-reproducible, are
:mod:`.source_maps`'.

Not done: reliability from negative detections; mask dilation; bit-reproducible sums of the spectra;
sources across polarizations; Gaussian or busy-function fits to the spectra; cubes across several GPUs.
Why these rules, and what the kernels cost, is DESIGN.md 5.32.
"""
import ctypes
import math

import numpy as np

from . import accel, smooth
from ._lib import lib, check, SourceLineTable
from .cube_operator import (AXES, MAX_CHANNELS, CubeOperator, CubeTemplate, SpectralCube, _rest_frequency,
                            channel_pitch, host_filled, is_bool, velocities)
from .link import _labels

MAX_TOTAL = 2 ** 31 - 2
_UNITS = ('beam', 'pixel')
_DOUBLE_FIELDS = ('flux', 'flux_err', 'peak', 'centroid', 'w50', 'w20', 'w50_lo', 'w50_hi', 'w20_lo', 'w20_hi')
_INT_FIELDS = ('peak_channel', 'channels')
#: what ``source_lines_host`` returns and ``kimg_source_lines`` fills, a row per source
LINE_TABLE_DTYPE = np.dtype([(name, np.float64) for name in _DOUBLE_FIELDS]
                            + [(name, np.int32) for name in _INT_FIELDS])
#: a row of the lines that the operator returns
LINES_DTYPE = np.dtype([('id', np.int32), ('flux', np.float64), ('flux_err', np.float64),
                        ('peak', np.float64), ('peak_channel', np.int32), ('centroid', np.float64),
                        ('w50', np.float64), ('w20', np.float64), ('w50_lo', np.float64),
                        ('w50_hi', np.float64), ('w20_lo', np.float64), ('w20_hi', np.float64),
                        ('channels', np.int32)])


def ragged(c0, c1):
    """``(c0, offsets)`` int32 of the ragged layout for sources whose ranges are ``c0 .. c1`` inclusive
    (the catalogue's columns)."""
    c0 = np.ascontiguousarray(c0, np.int32)
    c1 = np.asarray(c1, np.int64)
    if c0.ndim != 1 or c1.shape != c0.shape:
        raise ValueError('c0 and c1 must be [N]')
    lengths = c1 - c0 + 1
    if len(c0) and (c0.min() < 0 or lengths.min() < 1 or c1.max() >= MAX_CHANNELS):
        raise ValueError('a channel range is empty or leaves the band')
    total = int(lengths.sum())
    if total > MAX_TOTAL:
        raise ValueError('more than 2^31 - 2 entries')
    offsets = np.zeros(len(c0) + 1, np.int32)
    offsets[1:] = np.cumsum(lengths)
    return c0, offsets


def _layout(c0, offsets):
    c0 = np.asarray(c0)
    offsets = np.asarray(offsets)
    if c0.dtype != np.int32 or offsets.dtype != np.int32 or c0.ndim != 1 or offsets.shape != (len(c0) + 1,):
        raise ValueError('c0 must be int32 [N] and offsets int32 [N + 1]')
    return c0, offsets


def source_spectra_host(labels, cube, filled, c0, offsets):
    """The contract of ``kimg_cube_source_spectra`` in numpy: ``(sum, voxels, finite)``, float64 and two
    int32 arrays of ``offsets[-1]`` entries.  The sums run in ascending dense index."""
    labels = _labels(labels)
    cube = np.asarray(cube)
    if cube.dtype != np.float32 or cube.shape != labels.shape:
        raise ValueError('cube must be float32 of the shape of labels')
    filled = host_filled(filled, labels.shape[0])
    c0, offsets = _layout(c0, offsets)
    N = len(c0)
    total = int(offsets[-1])
    if total < 0:
        raise ValueError('a negative total')
    member = (labels > 0) & (labels <= N) & filled.reshape(-1, 1, 1, 1)
    d = np.flatnonzero(member.reshape(-1))              # ascending dense index
    s = labels.reshape(-1)[d].astype(np.int64) - 1
    c = d // int(np.prod(labels.shape[1:], dtype=np.int64))
    first = c0.astype(np.int64)[s]
    at = offsets.astype(np.int64)[s] + (c - first)
    inside = (c >= first) & (at < offsets.astype(np.int64)[s + 1]) & (at >= 0) & (at < total)
    d, at = d[inside], at[inside]
    f = cube.reshape(-1)[d]
    voxels = np.bincount(at, minlength=total).astype(np.int32)
    ok = np.isfinite(f)
    finite = np.bincount(at[ok], minlength=total).astype(np.int32)
    total_sum = np.zeros(total, np.float64)
    np.add.at(total_sum, at[ok], f[ok].astype(np.float64))     # (unbuffered: one by one, in the order given)
    return total_sum, voxels, finite


def _channel_tables(tables, C):
    try:
        unit, width, coord, variance = tables
    except (TypeError, ValueError):
        raise ValueError('tables must be (unit, width, coord, variance)') from None
    out = tuple(np.ascontiguousarray(t, np.float64) for t in (unit, width, coord, variance))
    for t in out:
        if t.shape != (C,):
            raise ValueError('every table must have one entry per channel')
    return out


def _quiet(x):
    return np.float64(np.nan) if x != x else np.float64(x)


def _edges(d, x, L):
    n = len(d)
    k = 0
    while k < n - 1 and not d[k] >= L:
        k += 1
    lo = x[0] if k == 0 else x[k - 1] + (((L - d[k - 1]) / (d[k] - d[k - 1])) * (x[k] - x[k - 1]))
    k = n - 1
    while k > 0 and not d[k] >= L:
        k -= 1
    hi = x[n - 1] if k == n - 1 else x[k + 1] + (((L - d[k + 1]) / (d[k] - d[k + 1])) * (x[k] - x[k + 1]))
    return lo, hi


def source_lines_host(c0, offsets, total_sum, finite, tables):
    """The contract of ``kimg_source_lines`` in numpy: a :data:`LINE_TABLE_DTYPE` array with a row per
    source.  ``tables`` = (unit, width, coord, variance), float64 [C] each."""
    c0, offsets = _layout(c0, offsets)
    total_sum = np.asarray(total_sum)
    finite = np.asarray(finite)
    if total_sum.dtype != np.float64 or finite.dtype != np.int32 or total_sum.ndim != 1 \
            or finite.shape != total_sum.shape:
        raise ValueError('sum must be float64 and finite int32, of one length')
    C = len(np.atleast_1d(tables[0]))
    unit, width, coord, variance = _channel_tables(tables, C)
    total = len(total_sum)
    nan = np.float64(np.nan)
    out = np.zeros(len(c0), LINE_TABLE_DTYPE)
    with np.errstate(all='ignore'):
        for s in range(len(c0)):
            first, start = int(c0[s]), int(offsets[s])
            n = int(offsets[s + 1]) - start
            if first < 0 or start < 0 or n < 0 or first + n > C or start + n > total:
                n = 0
            d = total_sum[start:start + n] * unit[first:first + n]
            x = coord[first:first + n]
            count = finite[start:start + n]
            flux = var = s0 = s1 = np.float64(0.0)
            peak, peak_k = nan, -1
            for k in range(n):
                flux = flux + d[k] * width[first + k]
                var = var + np.float64(count[k]) * variance[first + k]
                s0 = s0 + d[k]
                s1 = s1 + d[k] * x[k]
                if count[k] > 0 and (peak_k < 0 or d[k] > peak):
                    peak, peak_k = d[k], k
            edges = [nan] * 4
            if peak_k >= 0 and peak > 0.0:
                edges[0:2] = _edges(d, x, np.float64(0.5) * peak)
                edges[2:4] = _edges(d, x, np.float64(0.2) * peak)
            row = out[s]
            row['flux'] = _quiet(flux)
            row['flux_err'] = _quiet(np.sqrt(var))
            row['peak'] = _quiet(peak)
            row['peak_channel'] = -1 if peak_k < 0 else first + peak_k
            row['centroid'] = nan if s0 == 0.0 else _quiet(s1 / s0)
            row['w50'] = _quiet(np.abs(edges[1] - edges[0]))
            row['w20'] = _quiet(np.abs(edges[3] - edges[2]))
            for name, edge in zip(('w50_lo', 'w50_hi', 'w20_lo', 'w20_hi'), edges):
                row[name] = _quiet(edge)
            row['channels'] = n
    return out


def _axis(axis, rest_frequency, units):
    if axis not in AXES:
        raise ValueError("axis must be 'velocity' or 'frequency'")
    if rest_frequency is not None:
        if is_bool(rest_frequency):
            raise ValueError('rest_frequency must be a number, not a bool')
        rest_frequency = _rest_frequency(rest_frequency)
    if units not in _UNITS:
        raise ValueError("units must be 'beam' or 'pixel'")
    return axis, rest_frequency, units


def beam_area(beam):
    """``Omega = 2 pi sqrt(det Sigma)`` of a :class:`beam.Beam`, in pixels."""
    sigma = smooth.beam_covariance(beam)
    return 2.0 * math.pi * math.sqrt(sigma[0, 0] * sigma[1, 1] - sigma[0, 1] * sigma[1, 0])


def line_tables(the_cube, axis='velocity', rest_frequency=None, units='beam'):
    """``(unit, width, coord, variance)``, float64 [C] each, of a :class:`cube.SpectralCube` for
    :func:`source_lines_host` and the operator.  ``coord`` is ``the_cube.coordinates(axis,
    rest_frequency)``; ``width[c]`` half the absolute distance between the neighbours of channel c, the
    distance to its one neighbour at the ends of the band, and ``|channel_width|`` on the axis for a cube
    of one channel (refused without one).  ``units='beam'``: ``unit[c] = 1 / Omega_c``, the beam area
    in pixels of ``common_beam`` or else of ``beams[c]`` (a filled channel without a beam is refused);
    ``'pixel'``: 1, and Omega = 1.  ``variance[c] = Omega_c * (noise[c] * unit[c] * width[c])^2``, NaN
    where no noise is recorded.  Channels that are not filled have unit 0 and variance 0."""
    if not isinstance(the_cube, SpectralCube):
        raise TypeError('line_tables takes a SpectralCube')
    axis, rest_frequency, units = _axis(axis, rest_frequency, units)
    coord = np.ascontiguousarray(the_cube.coordinates(axis, rest_frequency), np.float64)
    C = len(coord)
    if C > 1:
        width = np.empty(C, np.float64)
        width[1:-1] = np.abs(coord[2:] - coord[:-2]) / 2.0
        width[0] = abs(coord[1] - coord[0])
        width[-1] = abs(coord[-1] - coord[-2])
    else:
        one = the_cube.axis_channel_width(axis, rest_frequency)
        if one is None:
            raise ValueError('a cube of one channel needs the channel width')
        width = np.array([abs(float(one))], np.float64)
    filled = the_cube.filled != 0
    omega = np.ones(C, np.float64)
    if units == 'beam':
        if the_cube.common_beam is not None:
            omega[:] = beam_area(the_cube.common_beam)
        else:
            for c in np.flatnonzero(filled):
                if the_cube.beams[c] is None:
                    raise ValueError('channel {} is filled and has no beam'.format(int(c)))
                omega[c] = beam_area(the_cube.beams[c])
    unit = np.where(filled, 1.0 / omega, 0.0)
    noise = np.asarray(the_cube.noise, np.float64)
    with np.errstate(invalid='ignore'):
        variance = np.where(filled, omega * (noise * unit * width) ** 2, 0.0)
    return unit, width, coord, variance


class SourceParameters:
    """``axis``: 'velocity' (radio convention, km/s, needs ``rest_frequency`` in Hz) or 'frequency'
    (Hz): the axis of widths, centroids and the flux's second unit.  ``units``: 'beam' (the cube is in
    Jy/beam: sums are divided by the beam area) or 'pixel' (sums as they are)."""

    def __init__(self, axis='velocity', rest_frequency=None, units='beam'):
        self.axis, self.rest_frequency, self.units = _axis(axis, rest_frequency, units)
        if self.axis == 'velocity' and self.rest_frequency is None:
            raise ValueError('the velocity axis needs a rest frequency')

    def __repr__(self):
        return 'SourceParameters(axis={!r}, rest_frequency={!r}, units={!r})'.format(
            self.axis, self.rest_frequency, self.units)


class SourceSpectra:
    """The ragged spectra of one :class:`Sources` call: ``sum`` (float64), ``voxels`` and ``finite``
    (int32), device arrays of ``total`` entries; ``c0`` and ``offsets`` (host int32 [N] and [N + 1]) say
    which entries are whose.  ``ready`` fires when the call has written them; :meth:`get` makes its
    queue wait for that on the device first."""

    def __init__(self, c0, offsets, tables, ready):
        self.c0 = c0
        self.offsets = offsets
        self.total = int(offsets[-1])
        self.sum, self.voxels, self.finite = tables
        self.ready = ready
        self._host = None

    def __len__(self):
        return len(self.c0)

    def get(self, command_queue):
        """``(sum, voxels, finite)`` as host arrays of ``total`` entries."""
        if self._host is None:
            if self.total == 0:
                self._host = (np.zeros(0, np.float64), np.zeros(0, np.int32), np.zeros(0, np.int32))
            else:
                if self.ready is not None:
                    command_queue.enqueue_wait_for_events([self.ready])
                self._host = tuple(t.get(command_queue) for t in (self.sum, self.voxels, self.finite))
        return self._host

    def spectrum(self, source, command_queue=None):
        """``(channels, sum, voxels, finite)`` of source ``source`` (1 to N)."""
        if is_bool(source) or not isinstance(source, (int, np.integer)) or not 1 <= source <= len(self):
            raise ValueError('source must be 1 to {}'.format(len(self)))
        queue = self._queue if command_queue is None else command_queue
        a, b = int(self.offsets[source - 1]), int(self.offsets[source])
        channels = int(self.c0[source - 1]) + np.arange(b - a)
        return (channels,) + tuple(t[a:b].copy() for t in self.get(queue))


class Sources(CubeOperator):
    """The parameteriser for cubes of shape ``cube_shape`` = (C, P, H, W).  ``op(labels, the_cube,
    catalogue)`` takes a :class:`link.LabelCube`, a :class:`cube.SpectralCube` and the catalogue of
    :class:`link.Link` (its ``id``, ``c0`` and ``c1`` are read); ``op(labels, array, catalogue,
    filled=..., tables=...)`` takes a plain float32 :class:`accel.DeviceArray` whose [P][H][W] plane is
    dense, with ``tables`` = (unit, width, coord, variance) as :func:`line_tables` makes them, or
    ``frequencies=`` [C] instead, from which coord and width are made with unit 1 and variance NaN.
    It returns ``(spectra, lines)``: a :class:`SourceSpectra` and a :data:`LINES_DTYPE` array.

    A call allocates the ragged tables, uploads ``c0`` and ``offsets`` (8 bytes a source), enqueues the
    two entries on ``command_queue`` after the labels' ``ready`` and waits for their results once, when it
    reads the lines.  An empty catalogue returns empty
    results without a launch."""

    def __init__(self, template, command_queue, cube_shape):
        super().__init__(template, command_queue, cube_shape, band=True)
        C, P, H, W = self.cube_shape
        if C * P * H * W > 2 ** 31 - 2:
            raise ValueError('more than 2^31 - 2 voxels: labels are int32')
        self._channel_tables = accel.DeviceArray(command_queue.context, (4 * C,), np.float64,
                                                 queue=command_queue)

    def _tables_from_frequencies(self, frequencies):
        params = self.params
        C = self.cube_shape[0]
        frequencies = np.asarray(frequencies, np.float64)
        if frequencies.shape != (C,):
            raise ValueError('frequencies must have one entry per channel')
        if C < 2:
            raise ValueError('a cube of one channel needs tables: its channel width is not known')
        coord = frequencies.copy()
        if params.axis == 'velocity':
            coord = velocities(frequencies, params.rest_frequency)
        width = np.empty(C, np.float64)
        width[1:-1] = np.abs(coord[2:] - coord[:-2]) / 2.0
        width[0] = abs(coord[1] - coord[0])
        width[-1] = abs(coord[-1] - coord[-2])
        return np.ones(C), width, coord, np.full(C, np.nan)

    def __call__(self, labels, cube, catalogue, filled=None, frequencies=None, tables=None):
        params = self.params
        C, P, H, W = self.cube_shape
        M = P * H * W
        queue = self.command_queue
        labels, array = self._arrays((labels, 'labels', np.int32), (cube, 'cube', np.float32))
        filled = self._own_filled(cube, filled, frequencies=frequencies, tables=tables)
        if isinstance(cube, SpectralCube):
            tables = line_tables(cube, params.axis, params.rest_frequency, params.units)
        else:
            if (tables is None) == (frequencies is None):
                raise ValueError('a plain array needs either tables or frequencies')
            if tables is None:
                tables = self._tables_from_frequencies(frequencies)
        tables = _channel_tables(tables, C)
        filled = self._filled(filled)
        catalogue = np.asarray(catalogue)
        if catalogue.ndim != 1 or catalogue.dtype.names is None \
                or not {'c0', 'c1'} <= set(catalogue.dtype.names):
            raise ValueError('catalogue must be a structured array with c0 and c1')
        c0, offsets = ragged(catalogue['c0'], catalogue['c1'])
        N = len(c0)
        if N and int(catalogue['c1'].max()) >= C:
            raise ValueError('a source of the catalogue leaves the band')
        total = int(offsets[-1])
        lines = np.zeros(N, LINES_DTYPE)
        lines['id'] = catalogue['id'] if 'id' in catalogue.dtype.names else np.arange(1, N + 1)
        if N == 0:
            empty = SourceSpectra(c0, offsets, (None, None, None), None)
            empty._queue = queue
            return empty, lines
        pitch = channel_pitch(array)
        label_pitch = channel_pitch(labels)
        self._wait_ready(labels)
        labels.used_on(queue)
        array.used_on(queue)
        context = queue.context
        # [c0 (N)][offsets (N + 1)] in one array, one upload
        layout = accel.DeviceArray(context, (2 * N + 1,), np.int32, queue=queue)
        layout.set_async(queue, np.concatenate((c0, offsets)))
        c0_ptr, offsets_ptr = layout.ptr, layout.ptr + 4 * N
        ragged_tables = (accel.DeviceArray(context, (total,), np.float64, queue=queue),
                         accel.DeviceArray(context, (total,), np.int32, queue=queue),
                         accel.DeviceArray(context, (total,), np.int32, queue=queue))
        # the rows: one buffer, so that one read brings everything: the float64 fields, then the int32 ones
        rows = accel.DeviceArray(context, (N * (8 * len(_DOUBLE_FIELDS) + 4 * len(_INT_FIELDS)),), np.uint8,
                                 queue=queue)
        at = {}
        for k, name in enumerate(_DOUBLE_FIELDS):
            at[name] = 8 * N * k
        for k, name in enumerate(_INT_FIELDS):
            at[name] = 8 * N * len(_DOUBLE_FIELDS) + 4 * N * k
        struct = SourceLineTable(**{name: rows.ptr + where for name, where in at.items()})
        handle = queue.handle
        check(lib().kimg_cube_source_spectra(
            labels.ptr, label_pitch, array.ptr, pitch, C, M, filled.ctypes.data_as(ctypes.c_void_p), N,
            c0_ptr, offsets_ptr, total, ragged_tables[0].ptr, ragged_tables[1].ptr, ragged_tables[2].ptr,
            handle), 'kimg_cube_source_spectra')
        ready = queue.enqueue_marker()
        host_ptr = lambda t: t.ctypes.data_as(ctypes.c_void_p)
        check(lib().kimg_source_lines(
            N, c0_ptr, offsets_ptr, total, ragged_tables[0].ptr, ragged_tables[2].ptr, C,
            host_ptr(tables[0]), host_ptr(tables[1]), host_ptr(tables[2]), host_ptr(tables[3]),
            self._channel_tables.ptr, ctypes.byref(struct), handle), 'kimg_source_lines')
        raw = rows.get(queue)                       # (the call's only wait)
        for name, where in at.items():
            dtype = LINE_TABLE_DTYPE[name]
            lines[name] = raw[where:where + dtype.itemsize * N].view(dtype)
        spectra = SourceSpectra(c0, offsets, ragged_tables, ready)
        spectra._queue = queue
        spectra._layout = layout
        return spectra, lines


class SourcesTemplate(CubeTemplate):
    params_type = SourceParameters
    operator = Sources
