"""Shared by test_link_host.py and test_link_gpu.py: a plain-Python restatement of the "Source linking"
contracts of include/kimg.h (a flood fill over an explicit neighbour list, math.fsum for the sums), the
masks and cubes of the tests, and the C ABI's rejections."""
import ctypes
import math

import numpy as np

from helpers import SENTINELS

EINVAL = -10001
EUNSUPPORTED = -10002
REACHES = tuple((xy, z) for xy in (0, 1, 2, 4, 9) for z in (0, 1, 2, 3))
INT_FIELDS = ('first', 'voxels', 'finite', 'c0', 'c1', 'y0', 'y1', 'x0', 'x1', 'peak_index', 'trough_index')
SUM_FIELDS = ('sum', 'sum_c', 'sum_y', 'sum_x')


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8)


def assert_same_bits(got, want, where=None):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (where, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(bits(got), bits(want)):
        bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
        assert False, (where, len(bad), bad[:5], got.reshape(-1)[bad[:5]], want.reshape(-1)[bad[:5]])


def key(value):
    """kimg_cube_stats' order of a float32 value: -0 below +0."""
    b = int(np.array([value], np.float32).view(np.uint32)[0])
    return b ^ (0xffffffff if b >> 31 else 0x80000000)


def restate(mask, filled, cube, reach_xy_sq, reach_z):
    """Voxel by voxel: (labels, N0, rows), rows a list of dicts with every field of the contract, the
    four sums by math.fsum, and 'abs' = [sum |term|] of each sum for the bound."""
    C, P, H, W = mask.shape
    on = {(c, p, y, x) for c in range(C) if filled[c] for p in range(P) for y in range(H) for x in range(W)
          if mask[c, p, y, x]}
    steps = [(dz, dy, dx) for dz in range(-reach_z, reach_z + 1) for dy in range(-3, 4) for dx in range(-3, 4)
             if dx * dx + dy * dy <= reach_xy_sq and (dz, dy, dx) != (0, 0, 0)]
    labels = np.zeros(mask.shape, np.int32)
    rows = []
    for start in sorted(on):                    # (tuples sort like the dense index)
        if labels[start]:
            continue
        number = len(rows) + 1
        labels[start] = number
        stack, members = [start], []
        while stack:
            c, p, y, x = v = stack.pop()
            members.append(v)
            for dz, dy, dx in steps:
                w = (c + dz, p, y + dy, x + dx)
                if w in on and not labels[w]:
                    labels[w] = number
                    stack.append(w)
        members.sort()
        dense = lambda v: ((v[0] * P + v[1]) * H + v[2]) * W + v[3]
        finite = [v for v in members if cube is not None and math.isfinite(cube[v])]
        row = dict(first=dense(members[0]), voxels=len(members), finite=len(finite),
                   c0=min(v[0] for v in members), c1=max(v[0] for v in members),
                   y0=min(v[2] for v in members), y1=max(v[2] for v in members),
                   x0=min(v[3] for v in members), x1=max(v[3] for v in members),
                   peak=np.float32(np.nan), trough=np.float32(np.nan), peak_index=-1, trough_index=-1)
        if finite:
            top = min(finite, key=lambda v: (-key(cube[v]), dense(v)))
            low = min(finite, key=lambda v: (key(cube[v]), dense(v)))
            row.update(peak=cube[top], peak_index=dense(top), trough=cube[low], trough_index=dense(low))
        sums, magnitudes = [], []
        for axis in (None, 0, 2, 3):
            terms = [float(cube[v]) * (1.0 if axis is None else float(v[axis])) for v in finite]
            sums.append(math.fsum(terms))
            magnitudes.append(math.fsum(abs(t) for t in terms))
        row.update(sum=sums[0], sum_c=sums[1], sum_y=sums[2], sum_x=sums[3], abs=magnitudes)
        rows.append(row)
    return labels, len(rows), rows


def assert_table(table, rows, where=None, exact_sums=True):
    """A measured table (link.TABLE_DTYPE) against restate()'s rows: integer fields and peaks by bits;
    the sums equal, or within n * 2^-53 * sum |term| of the fsum."""
    assert len(table) == len(rows), (where, len(table), len(rows))
    for s, row in enumerate(rows):
        for name in INT_FIELDS:
            assert table[name][s] == row[name], (where, s, name, table[name][s], row[name])
        for name in ('peak', 'trough'):
            assert_same_bits(table[name][s], np.float32(row[name]), (where, s, name))
        for k, name in enumerate(SUM_FIELDS):
            got, want = float(table[name][s]), row[name]
            if exact_sums:
                assert got == want, (where, s, name, got, want)
            else:
                assert abs(got - want) <= row['finite'] * 2.0 ** -53 * row['abs'][k], (where, s, name, got, want)


def random_mask(shape, seed, density, values=(1,)):
    rng = np.random.default_rng(seed)
    on = rng.random(shape) < density
    return np.where(on, rng.choice(np.array(values, np.uint8), size=shape), 0).astype(np.uint8)


def filled_for(C, turn):
    """All filled on even turns; on odd ones the middle channel (C >= 3) or none is left out."""
    filled = np.ones(C, np.uint8)
    if turn % 2 and C >= 3:
        filled[C // 2] = 0
    return filled


def integer_cube(shape, seed):
    """Integers below 2^10 in magnitude, with NaN, Inf, -0 and ties sprinkled in: every order of a sum
    of them (times an index below 2^12) is exact."""
    rng = np.random.default_rng(seed)
    cube = rng.integers(-1023, 1024, size=shape).astype(np.float32)
    flat = cube.reshape(-1)
    for value, share in ((np.nan, 0.05), (np.inf, 0.01), (-np.inf, 0.01), (-0.0, 0.03), (1023.0, 0.03),
                         (-1023.0, 0.03)):
        flat[rng.random(flat.size) < share] = value
    return cube


def gaussian_cube(shape, seed):
    rng = np.random.default_rng(seed)
    cube = rng.standard_normal(shape).astype(np.float32)
    cube.reshape(-1)[rng.random(cube.size) < 0.03] = np.nan
    return cube


def checkerboard(shape):
    """Every voxel its own source at reach (1, 0): (y + x) even."""
    C, P, H, W = shape
    y, x = np.mgrid[:H, :W]
    return np.broadcast_to(((y + x) % 2 == 0).astype(np.uint8), shape).copy()


def serpentine(C, H, W):
    """One chain through a (1, H, W) plane and up through the channels at reach (1, 1): even rows are
    set whole, odd rows only at one end, alternating; the end of a channel's path joins the next
    channel through the voxel above it.  Channels alternate direction so that the chain is one path."""
    mask = np.zeros((C, 1, H, W), np.uint8)
    plane = np.zeros((H, W), np.uint8)
    plane[0::2] = 1
    for k, y in enumerate(range(1, H, 2)):
        plane[y, W - 1 if k % 2 == 0 else 0] = 1
    mask[:, 0] = plane
    # two channels' paths touch everywhere, so cut all links but one: leave out every other channel's
    # plane except a single voxel that bridges its neighbours
    rows = (H + 1) // 2                     # the path ends in the last even row, at this x
    end = (H - 1) // 2 * 2, (W - 1 if rows % 2 else 0)
    for c in range(1, C, 2):
        bridge = np.zeros((H, W), np.uint8)
        bridge[end if (c // 2) % 2 == 0 else (0, 0)] = 1
        mask[c, 0] = bridge
    return mask


def combs(C, plane):
    """Teeth along the channel axis on every other pixel of every other row, joined only in the last
    channel, where the whole plane is set: one source per polarization whose smallest index is
    reached through the last channel."""
    P, H, W = plane
    mask = np.zeros((C, P, H, W), np.uint8)
    mask[:, :, 0::2, 0::2] = 1
    mask[C - 1] = 1
    return mask


def u_shape():
    """The smallest dense index of the right arm is reached only through the bottom row."""
    mask = np.zeros((1, 1, 5, 5), np.uint8)
    mask[0, 0, :, 0] = 1
    mask[0, 0, :, 4] = 1
    mask[0, 0, 4, :] = 1
    return mask


def spiral(n=9):
    """A path that winds inwards from (0, 0) with a gap of one pixel between its turns: one source at
    reach 1, and the inner turns' smallest indices are reached only through the outer ones."""
    mask = np.zeros((1, 1, n, n), np.uint8)
    plane = mask[0, 0]
    y = x = 0
    dy, dx = 0, 1
    plane[0, 0] = 1

    def free(y, x):
        return not (0 <= y < n and 0 <= x < n and plane[y, x])

    while True:
        for _ in range(2):
            ny, nx = y + dy, x + dx
            if 0 <= ny < n and 0 <= nx < n and free(ny, nx) and free(ny + dy, nx + dx):
                break
            dy, dx = dx, -dy
        else:
            return mask
        y, x = ny, nx
        plane[y, x] = 1


# ---- the device runs (nothing of the package is imported until one is made) --------------------------

FLOAT_LAYOUTS = ((0, 0), (3, 0), (4, 0), (0, 1))
MASK_LAYOUTS = ((0, 0), (1, 0), (4, 0), (3, 0), (0, 1))
LABEL_LAYOUTS = ((0, 0), (1, 0), (4, 0), (0, 1))
SENTINEL = {np.dtype(np.float32): SENTINELS[np.dtype(np.float32)], np.dtype(np.uint8): np.uint8(0xa5),
            np.dtype(np.int32): SENTINELS[np.dtype(np.int32)], np.dtype(np.float64): SENTINELS[np.dtype(np.float64)]}


class Padded:
    """[C][M] inside a flat device buffer of sentinels: `offset` elements in, channel pitch M + pad.
    `inner` None: sentinels throughout (a target)."""

    def __init__(self, ctx, q, C, M, inner, pad, offset, dtype):
        from katsdpimager_amd import accel
        self.C, self.M, self.pitch, self.offset = C, M, M + pad, offset
        self.dtype = np.dtype(dtype)
        self.host = np.full(offset + C * self.pitch, SENTINEL[self.dtype], self.dtype)
        if inner is not None:
            self.rows(self.host)[:, :M] = inner.reshape(C, M)
        self.whole = accel.DeviceArray(ctx, self.host.shape, self.dtype)
        self.whole.set(q, self.host)
        self.ptr = self.whole.ptr + offset * self.dtype.itemsize

    def rows(self, flat):
        return flat[self.offset:].reshape(self.C, self.pitch)

    def assert_holds(self, q, want, where):
        """The buffer holds `want` [C][M] and what it held before everywhere else."""
        expect = self.host.copy()
        self.rows(expect)[:, :self.M] = want.reshape(self.C, self.M)
        assert_same_bits(self.whole.get(q), expect, where)

    def assert_unchanged(self, q, where):
        assert np.array_equal(self.whole.get(q).view(np.uint8), self.host.view(np.uint8)), \
            (where, 'an input or its padding changed')


class Tables:
    """The device arrays of a kimg_catalogue with `rows` rows each, full of sentinels, and counts."""

    def __init__(self, ctx, q, rows):
        from katsdpimager_amd import accel, link, _lib
        self.rows = rows
        self.arrays = {}
        for name in link.TABLE_DTYPE.names:
            dtype = link.TABLE_DTYPE[name]
            array = accel.DeviceArray(ctx, (rows,), dtype)
            array.set(q, np.full(rows, SENTINEL[dtype], dtype))
            self.arrays[name] = array
        self.work = accel.DeviceArray(ctx, (3 * rows,), np.int64)
        self.counts = accel.DeviceArray(ctx, (2,), np.int32)
        self.counts.set(q, np.full(2, SENTINEL[np.dtype(np.int32)], np.int32))
        self.struct = _lib.Catalogue(work=self.work.ptr, **{n: a.ptr for n, a in self.arrays.items()})

    def get(self, q):
        from katsdpimager_amd import link
        table = np.zeros(self.rows, link.TABLE_DTYPE)
        for name, array in self.arrays.items():
            table[name] = array.get(q)
        return table

    def assert_untouched(self, table, start, where):
        for name in table.dtype.names:
            dtype = table.dtype[name]
            want = np.full(len(table) - start, SENTINEL[dtype], dtype)
            assert_same_bits(np.ascontiguousarray(table[name][start:]), want, (where, name, 'rows beyond'))


def host_ptr(array):
    return array.ctypes.data_as(ctypes.c_void_p)


def scratch(ctx, C, M):
    from katsdpimager_amd import accel, _lib
    return accel.DeviceArray(ctx, (_lib.lib().kimg_cube_link_scratch_bytes(C, M) // 4,), np.int32)


def fsum_rows(labels, cube, filled, rows):
    """Per source and sum: (math.fsum of the terms in float64, math.fsum of their magnitudes)."""
    C, P, H, W = labels.shape
    member = (labels > 0) & (np.asarray(filled).reshape(-1, 1, 1, 1) != 0) & np.isfinite(cube)
    d = np.flatnonzero(member.reshape(-1))
    s = labels.reshape(-1)[d] - 1
    order = np.argsort(s, kind='stable')
    d, s = d[order], s[order]
    f = cube.reshape(-1)[d].astype(np.float64)
    c = (d // (P * H * W)).astype(np.float64)
    y = (d % (H * W) // W).astype(np.float64)
    x = (d % W).astype(np.float64)
    cuts = np.searchsorted(s, np.arange(rows + 1))
    out = []
    for k in range(rows):
        a, b = cuts[k], cuts[k + 1]
        out.append([(math.fsum(t), math.fsum(np.abs(t))) for t in (f[a:b], f[a:b] * c[a:b], f[a:b] * y[a:b], f[a:b] * x[a:b])])
    return out


def assert_measured(got, want, labels, cube, filled, exact, where):
    """Integer fields and peaks by bits; sums equal (`exact`) or within the bound of the fsum."""
    for name in INT_FIELDS + ('peak', 'trough'):
        assert_same_bits(np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name]), (where, name))
    if exact:
        for name in SUM_FIELDS:
            assert_same_bits(np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name]), (where, name))
        return
    sums = fsum_rows(labels, cube, filled, len(want))
    for s in range(len(want)):
        for k, name in enumerate(SUM_FIELDS):
            exact_sum, magnitude = sums[s][k]
            bound = int(want['finite'][s]) * 2.0 ** -53 * magnitude
            assert abs(float(got[name][s]) - exact_sum) <= bound, (where, s, name, got[name][s], exact_sum, bound)


def run_case(ctx, q, mask, cube, filled, reach, minima, layouts, extra_rows=3, capacity=None):
    """link, measure, filter and label_mask of one case in every layout of `layouts` against the
    twins; the labels of all layouts are the same.  Returns N0."""
    from katsdpimager_amd import link, _lib
    lib = _lib.lib()
    s = q.handle
    C, P, H, W = mask.shape
    M = P * H * W
    want_labels, N0 = link.link_host(mask, filled, *reach)
    rows = N0 if capacity is None else min(N0, capacity)
    want_table = link.measure_host(want_labels, cube, filled, N0, capacity)
    exact = bool(np.all(cube[np.isfinite(cube)] == np.round(cube[np.isfinite(cube)])))
    if capacity is None:
        want_filtered, want_kept = link.filter_host(want_labels, want_table, *minima)
        t = want_table
        keep = ((t['voxels'] >= minima[0]) & (t['x1'] - t['x0'] + 1 >= minima[1])
                & (t['y1'] - t['y0'] + 1 >= minima[1]) & (t['c1'] - t['c0'] + 1 >= minima[2]))
        assert keep.sum() == len(want_kept)
    first = None
    for (fpad, foff), (mpad, moff), (lpad, loff) in layouts:
        at = (mask.shape, reach, (fpad, foff), (mpad, moff), (lpad, loff))
        the_mask = Padded(ctx, q, C, M, mask, mpad, moff, np.uint8)
        the_cube = Padded(ctx, q, C, M, cube, fpad, foff, np.float32)
        labels = Padded(ctx, q, C, M, None, lpad, loff, np.int32)
        work = scratch(ctx, C, M)
        tables = Tables(ctx, q, rows + extra_rows)
        room = rows + extra_rows if capacity is None else capacity
        _lib.check(lib.kimg_cube_link(the_mask.ptr, the_mask.pitch, labels.ptr, labels.pitch, C, P, H, W,
                                      host_ptr(filled), reach[0], reach[1], work.ptr, tables.counts.ptr, s),
                   'link')
        labels.assert_holds(q, want_labels, at + ('labels',))
        assert tables.counts.get(q)[0] == N0, at
        got_labels = labels.whole.get(q)
        if first is None:
            first = labels.rows(got_labels)[:, :M].copy()
        assert np.array_equal(labels.rows(got_labels)[:, :M], first), at + ('labels differ between layouts',)

        _lib.check(lib.kimg_cube_measure(labels.ptr, labels.pitch, the_cube.ptr, the_cube.pitch, C, P, H, W,
                                         host_ptr(filled), ctypes.byref(tables.struct), room,
                                         tables.counts.ptr, s), 'measure')
        got = tables.get(q)
        tables.assert_untouched(got, rows, at)
        assert_measured(got[:rows], want_table, want_labels, cube, filled, exact, at)
        labels.assert_holds(q, want_labels, at + ('labels after measure',))

        if capacity is None:
            _lib.check(lib.kimg_cube_link_filter(labels.ptr, labels.pitch, C, M, ctypes.byref(tables.struct),
                                                 room, *minima, tables.counts.ptr, s), 'filter')
            labels.assert_holds(q, want_filtered, at + ('filtered labels', minima))
            after = tables.get(q)
            N = len(want_kept)
            assert list(tables.counts.get(q)) == [N0, N], at
            assert_same_bits(after[:N], got[:rows][keep], at + ('rows after the filter',))
            assert_same_bits(after[N:], got[N:], at + ('rows behind the kept ones',))
            final = want_filtered
        else:
            # more sources than rows: the filter changes nothing
            _lib.check(lib.kimg_cube_link_filter(labels.ptr, labels.pitch, C, M, ctypes.byref(tables.struct),
                                                 room, 2, 1, 1, tables.counts.ptr, s), 'filter')
            labels.assert_holds(q, want_labels, at + ('labels after a filter without rows',))
            assert list(tables.counts.get(q)) == [N0, N0], at
            assert_same_bits(tables.get(q), got, at + ('rows after a filter without rows',))
            final = want_labels

        for source in (0, max(1, int(final.max()) // 2)):
            out = Padded(ctx, q, C, M, None, mpad, moff, np.uint8)
            _lib.check(lib.kimg_cube_label_mask(labels.ptr, labels.pitch, out.ptr, out.pitch, C, M, source, s),
                       'label_mask')
            out.assert_holds(q, link.label_mask_host(final, source), at + ('label_mask', source))
        the_mask.assert_unchanged(q, at)
        the_cube.assert_unchanged(q, at)
    return N0


def layouts(count=5):
    return [(FLOAT_LAYOUTS[k % 4], MASK_LAYOUTS[k % 5], LABEL_LAYOUTS[k % 4]) for k in range(count)]


def abi_rejections(lib, catalogue_type, mask, labels, cube, scratch, counts, tables, filled, stream=None):
    """[(name, got, want)] for the argument checks of the six entries.  mask, labels, cube: device
    pointers (c_void_p) of dense [4][16] arrays; tables: a device pointer with room for every array of
    a catalogue of 8 rows, 8 bytes each."""
    P = ctypes.c_void_p
    plus = lambda p, n: P(p.value + n)
    good = catalogue_type(**{name: tables.value + 64 * k for k, (name, _) in enumerate(catalogue_type._fields_)})
    null_field = catalogue_type(**{name: (0 if name == 'peak' else tables.value + 64 * k)
                                   for k, (name, _) in enumerate(catalogue_type._fields_)})
    odd_field = catalogue_type(**{name: tables.value + 64 * k + (4 if name == 'sum_y' else 0)
                                  for k, (name, _) in enumerate(catalogue_type._fields_)})
    ref = ctypes.byref
    calls = []

    def link(want, mask=mask, mask_pitch=16, labels=labels, label_pitch=16, C=4, shape=(1, 4, 4),
             filled=filled, reach=(1, 1), scratch=scratch, counts=counts):
        calls.append(('link', lib.kimg_cube_link(mask, mask_pitch, labels, label_pitch, C, *shape, filled,
                                                 reach[0], reach[1], scratch, counts, stream), want))

    link(0)
    for name in ('mask', 'labels', 'filled', 'scratch', 'counts'):
        link(EINVAL, **{name: None})
    link(EINVAL, C=0)
    link(EINVAL, shape=(0, 4, 4))
    link(EINVAL, shape=(1, 4, 0))
    link(EINVAL, mask_pitch=15)
    link(EINVAL, label_pitch=15)
    link(EINVAL, labels=plus(labels, 2))
    link(EINVAL, counts=plus(counts, 1))
    for reach in ((-1, 1), (10, 1), (1, -1), (1, 4)):
        link(EINVAL, reach=reach)
    link(EUNSUPPORTED, C=4097)
    link(EUNSUPPORTED, C=1, shape=(1, 46341, 46341), mask_pitch=2 ** 32, label_pitch=2 ** 32)

    def measure(want, labels=labels, label_pitch=16, cube=cube, pitch=16, C=4, shape=(1, 4, 4), filled=filled,
                catalogue=ref(good), capacity=8, counts=counts):
        calls.append(('measure', lib.kimg_cube_measure(labels, label_pitch, cube, pitch, C, *shape, filled,
                                                       catalogue, capacity, counts, stream), want))

    measure(0)
    for name in ('labels', 'cube', 'filled', 'catalogue', 'counts'):
        measure(EINVAL, **{name: None})
    measure(EINVAL, C=0)
    measure(EINVAL, shape=(1, 0, 4))
    measure(EINVAL, label_pitch=15)
    measure(EINVAL, pitch=15)
    measure(EINVAL, cube=plus(cube, 2))
    measure(EINVAL, capacity=0)
    measure(EINVAL, catalogue=ref(null_field))
    measure(EINVAL, catalogue=ref(odd_field))
    measure(EUNSUPPORTED, C=4097)

    def select(want, labels=labels, label_pitch=16, C=4, M=16, catalogue=ref(good), capacity=8,
               minima=(1, 1, 1), counts=counts):
        calls.append(('filter', lib.kimg_cube_link_filter(labels, label_pitch, C, M, catalogue, capacity,
                                                          *minima, counts, stream), want))

    select(0)
    select(0, M=0)
    for name in ('labels', 'catalogue', 'counts'):
        select(EINVAL, **{name: None})
    select(EINVAL, C=0)
    select(EINVAL, M=-1)
    select(EINVAL, label_pitch=15)
    select(EINVAL, capacity=0)
    for minima in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        select(EINVAL, minima=minima)
    select(EUNSUPPORTED, C=2, M=2 ** 30, label_pitch=2 ** 30)

    def label_mask(want, labels=labels, label_pitch=16, mask=mask, mask_pitch=16, C=4, M=16, source=0):
        calls.append(('label_mask', lib.kimg_cube_label_mask(labels, label_pitch, mask, mask_pitch, C, M,
                                                             source, stream), want))

    label_mask(0)
    label_mask(0, M=0)
    for name in ('labels', 'mask'):
        label_mask(EINVAL, **{name: None})
    label_mask(EINVAL, C=0)
    label_mask(EINVAL, M=-1)
    label_mask(EINVAL, label_pitch=15)
    label_mask(EINVAL, mask_pitch=15)
    label_mask(EINVAL, source=-1)
    label_mask(EINVAL, labels=plus(labels, 1))
    label_mask(EUNSUPPORTED, C=4097)

    calls.append(('scratch', lib.kimg_cube_link_scratch_bytes(4, 16), 4 * (4 + 4)))
    calls.append(('scratch', lib.kimg_cube_link_scratch_bytes(3, 1025), 4 * (6 + 4)))
    calls.append(('scratch', lib.kimg_cube_link_scratch_bytes(0, 16), 0))
    calls.append(('scratch', lib.kimg_cube_link_scratch_bytes(2, 2 ** 30), 0))
    calls.append(('work', lib.kimg_cube_catalogue_work_bytes(8), 192))
    calls.append(('work', lib.kimg_cube_catalogue_work_bytes(0), 0))
    return calls
