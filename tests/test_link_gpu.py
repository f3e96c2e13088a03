"""Source linking on the device (csrc/cube_link.hip) against the numpy twins (link.py, tested on their
own in test_link_host.py): the entries through the C ABI inside buffers of sentinels, the labels, the
counts, every integer field and the peaks by bits, the four sums equal on integer cubes and within
n * 2^-53 * sum |term| of math.fsum on Gaussian ones; then the operator end to end.

Layouts: the float pitch padded by 0, 3 and 4 floats and once more starting 1 float in; the mask pitch
padded by 0, 1, 4 and 3 bytes and once more starting 1 byte in; the label pitch padded by 0, 1 and 4
labels and once more starting 1 label in.  A workgroup of the dense launches holds 1024 elements of one
channel, so every case with C > 1 spans several, and (1, 5, 257) and (3, 33, 65) do so in one channel."""
import ctypes
import math

import numpy as np
import pytest

import link_cases as cases
from helpers import context_queue, SENTINELS

pytestmark = pytest.mark.gpu

CHANNELS = (1, 2, 3, 9, 33)
PLANES = ((1, 1, 1), (1, 3, 5), (2, 7, 9), (1, 5, 257), (3, 33, 65))
FLOAT_LAYOUTS = ((0, 0), (3, 0), (4, 0), (0, 1))
MASK_LAYOUTS = ((0, 0), (1, 0), (4, 0), (3, 0), (0, 1))
LABEL_LAYOUTS = ((0, 0), (1, 0), (4, 0), (0, 1))
DENSITIES = (0.01, 0.1, 0.45)
SENTINEL = {np.dtype(np.float32): SENTINELS[np.dtype(np.float32)], np.dtype(np.uint8): np.uint8(0xa5),
            np.dtype(np.int32): SENTINELS[np.dtype(np.int32)], np.dtype(np.float64): SENTINELS[np.dtype(np.float64)]}


class _Padded:
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
        cases.assert_same_bits(self.whole.get(q), expect, where)

    def assert_unchanged(self, q, where):
        assert np.array_equal(self.whole.get(q).view(np.uint8), self.host.view(np.uint8)), \
            (where, 'an input or its padding changed')


class _Tables:
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
            cases.assert_same_bits(np.ascontiguousarray(table[name][start:]), want, (where, name, 'rows beyond'))


def _host_ptr(array):
    return array.ctypes.data_as(ctypes.c_void_p)


def _scratch(ctx, C, M):
    from katsdpimager_amd import accel, _lib
    return accel.DeviceArray(ctx, (_lib.lib().kimg_cube_link_scratch_bytes(C, M) // 4,), np.int32)


def _fsum_rows(labels, cube, filled, rows):
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


def _assert_measured(got, want, labels, cube, filled, exact, where):
    """Integer fields and peaks by bits; sums equal (`exact`) or within the bound of the fsum."""
    for name in cases.INT_FIELDS + ('peak', 'trough'):
        cases.assert_same_bits(np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name]), (where, name))
    if exact:
        for name in cases.SUM_FIELDS:
            cases.assert_same_bits(np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name]), (where, name))
        return
    sums = _fsum_rows(labels, cube, filled, len(want))
    for s in range(len(want)):
        for k, name in enumerate(cases.SUM_FIELDS):
            exact_sum, magnitude = sums[s][k]
            bound = int(want['finite'][s]) * 2.0 ** -53 * magnitude
            assert abs(float(got[name][s]) - exact_sum) <= bound, (where, s, name, got[name][s], exact_sum, bound)


def _run_case(ctx, q, mask, cube, filled, reach, minima, layouts, extra_rows=3, capacity=None):
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
        the_mask = _Padded(ctx, q, C, M, mask, mpad, moff, np.uint8)
        the_cube = _Padded(ctx, q, C, M, cube, fpad, foff, np.float32)
        labels = _Padded(ctx, q, C, M, None, lpad, loff, np.int32)
        scratch = _scratch(ctx, C, M)
        tables = _Tables(ctx, q, rows + extra_rows)
        room = rows + extra_rows if capacity is None else capacity
        _lib.check(lib.kimg_cube_link(the_mask.ptr, the_mask.pitch, labels.ptr, labels.pitch, C, P, H, W,
                                      _host_ptr(filled), reach[0], reach[1], scratch.ptr, tables.counts.ptr, s),
                   'link')
        labels.assert_holds(q, want_labels, at + ('labels',))
        assert tables.counts.get(q)[0] == N0, at
        got_labels = labels.whole.get(q)
        if first is None:
            first = labels.rows(got_labels)[:, :M].copy()
        assert np.array_equal(labels.rows(got_labels)[:, :M], first), at + ('labels differ between layouts',)

        _lib.check(lib.kimg_cube_measure(labels.ptr, labels.pitch, the_cube.ptr, the_cube.pitch, C, P, H, W,
                                         _host_ptr(filled), ctypes.byref(tables.struct), room,
                                         tables.counts.ptr, s), 'measure')
        got = tables.get(q)
        tables.assert_untouched(got, rows, at)
        _assert_measured(got[:rows], want_table, want_labels, cube, filled, exact, at)
        labels.assert_holds(q, want_labels, at + ('labels after measure',))

        if capacity is None:
            _lib.check(lib.kimg_cube_link_filter(labels.ptr, labels.pitch, C, M, ctypes.byref(tables.struct),
                                                 room, *minima, tables.counts.ptr, s), 'filter')
            labels.assert_holds(q, want_filtered, at + ('filtered labels', minima))
            after = tables.get(q)
            N = len(want_kept)
            assert list(tables.counts.get(q)) == [N0, N], at
            cases.assert_same_bits(after[:N], got[:rows][keep], at + ('rows after the filter',))
            cases.assert_same_bits(after[N:], got[N:], at + ('rows behind the kept ones',))
            final = want_filtered
        else:
            # more sources than rows: the filter changes nothing
            _lib.check(lib.kimg_cube_link_filter(labels.ptr, labels.pitch, C, M, ctypes.byref(tables.struct),
                                                 room, 2, 1, 1, tables.counts.ptr, s), 'filter')
            labels.assert_holds(q, want_labels, at + ('labels after a filter without rows',))
            assert list(tables.counts.get(q)) == [N0, N0], at
            cases.assert_same_bits(tables.get(q), got, at + ('rows after a filter without rows',))
            final = want_labels

        for source in (0, max(1, int(final.max()) // 2)):
            out = _Padded(ctx, q, C, M, None, mpad, moff, np.uint8)
            _lib.check(lib.kimg_cube_label_mask(labels.ptr, labels.pitch, out.ptr, out.pitch, C, M, source, s),
                       'label_mask')
            out.assert_holds(q, link.label_mask_host(final, source), at + ('label_mask', source))
        the_mask.assert_unchanged(q, at)
        the_cube.assert_unchanged(q, at)
    return N0


def _layouts(count=5):
    return [(FLOAT_LAYOUTS[k % 4], MASK_LAYOUTS[k % 5], LABEL_LAYOUTS[k % 4]) for k in range(count)]


@pytest.mark.parametrize('C', CHANNELS)
def test_entries_against_twins(C):
    """Every plane at a density, a reach and filter minima that rotate with the plane and C; integer
    cubes (sums equal) and Gaussian ones (sums within the bound) alternate."""
    ctx, q = context_queue()
    for i, plane in enumerate(PLANES):
        turn = C + i
        shape = (C,) + plane
        mask = cases.random_mask(shape, 10 * C + i, DENSITIES[turn % 3], values=(1, 1, 2, 255))
        if mask.size < 4:
            mask[...] = 1
        cube = cases.integer_cube(shape, turn) if turn % 2 else cases.gaussian_cube(shape, turn)
        filled = cases.filled_for(C, turn)
        reach = ((1, 1), (2, 1), (1, 0), (4, 2), (9, 3))[turn % 5]
        minima = ((1, 1, 1), (3, 1, 1), (1, 2, 1), (2, 1, 2))[turn % 4]
        _run_case(ctx, q, mask, cube, filled, reach, minima, _layouts())


@pytest.mark.parametrize('density', DENSITIES)
def test_every_density_on_the_large_plane(density):
    ctx, q = context_queue()
    shape = (9, 3, 33, 65)
    mask = cases.random_mask(shape, 5, density)
    for k, cube in enumerate((cases.integer_cube(shape, 1), cases.gaussian_cube(shape, 2))):
        _run_case(ctx, q, mask, cube, cases.filled_for(9, k), (1, 1), (2, 2, 1), _layouts(2))


def test_every_reach():
    ctx, q = context_queue()
    shape = (9, 2, 7, 9)
    mask = cases.random_mask(shape, 3, 0.1)
    cube = cases.integer_cube(shape, 4)
    seen = set()
    for k, reach in enumerate(cases.REACHES):
        seen.add(_run_case(ctx, q, mask, cube, cases.filled_for(9, 1), reach, (1, 1, 1), _layouts(5)[k % 5:][:1]))
    assert len(seen) > 5


def test_all_set():
    """One source per polarization: every lane of the measure launch on one destination."""
    ctx, q = context_queue()
    for shape in ((3, 2, 7, 9), (2, 1, 5, 257), (9, 3, 33, 65)):
        mask = np.ones(shape, np.uint8)
        for k, cube in enumerate((cases.integer_cube(shape, 1), cases.gaussian_cube(shape, 2))):
            N0 = _run_case(ctx, q, mask, cube, np.ones(shape[0], np.uint8), (1, 1), (1, 1, 1),
                           _layouts(5)[2 * k:][:2])
            assert N0 == shape[1]


def test_checkerboard_above_capacity():
    """Every voxel its own source at reach (1, 0): more sources than rows.  The labels are exact, the
    rows up to the capacity are measured, nothing beyond them is written, a filter changes nothing;
    and the operator raises TooManySources with the full labels."""
    from katsdpimager_amd import accel, link
    ctx, q = context_queue()
    shape = (3, 1, 33, 65)
    mask = cases.checkerboard(shape)
    cube = cases.integer_cube(shape, 6)
    filled = np.ones(3, np.uint8)
    N0 = _run_case(ctx, q, mask, cube, filled, (1, 0), None, _layouts(2), extra_rows=5, capacity=1000)
    assert N0 == int(mask.sum()) > 1000
    op = link.LinkTemplate(ctx, link.LinkParameters(radius_xy=1, radius_z=0, max_sources=1000, min_voxels=2)
                           ).instantiate(q, shape)
    device_mask = accel.DeviceArray(ctx, shape, np.uint8)
    device_mask.set(q, mask)
    device_cube = accel.DeviceArray(ctx, shape, np.float32)
    device_cube.set(q, cube)
    with pytest.raises(link.TooManySources) as caught:
        op(device_mask, device_cube, filled=filled)
    assert caught.value.count == N0
    cases.assert_same_bits(caught.value.labels.get(q), link.link_host(mask, filled, 1, 0)[0])


def test_long_chains():
    """A serpentine through (1, 33, 65) and up through 33 channels, one chain of some 19000 voxels
    across every workgroup boundary; combs joined only in the last channel; a U and a spiral."""
    ctx, q = context_queue()
    mask = cases.serpentine(33, 33, 65)
    cube = cases.integer_cube(mask.shape, 8)
    assert _run_case(ctx, q, mask, cube, np.ones(33, np.uint8), (1, 1), (1, 1, 1), _layouts(2)) == 1
    assert _run_case(ctx, q, mask, cube, np.ones(33, np.uint8), (1, 0), (1, 1, 1), _layouts(1)) == 33
    for shape in ((9, 2, 7, 9), (33, 1, 5, 257)):
        mask = cases.combs(shape[0], shape[1:])
        cube = cases.gaussian_cube(shape, 9)
        assert _run_case(ctx, q, mask, cube, np.ones(shape[0], np.uint8), (1, 1), (1, 1, 1), _layouts(2)) == shape[1]
    for mask in (cases.u_shape(), cases.spiral(9), cases.spiral(33)):
        cube = cases.integer_cube(mask.shape, 2)
        assert _run_case(ctx, q, mask, cube, np.ones(1, np.uint8), (1, 0), (1, 1, 1), _layouts(2)) == 1


def test_abi_rejections():
    from katsdpimager_amd import accel, _lib
    ctx, q = context_queue()
    P = ctypes.c_void_p
    mask = _Padded(ctx, q, 4, 16, cases.random_mask((4, 16), 3, 0.3), 0, 0, np.uint8)
    cube = _Padded(ctx, q, 4, 16, cases.integer_cube((4, 16), 1), 0, 0, np.float32)
    labels = _Padded(ctx, q, 4, 16, None, 0, 0, np.int32)
    scratch = _scratch(ctx, 4, 16)
    counts = accel.DeviceArray(ctx, (2,), np.int32)
    tables = accel.DeviceArray(ctx, (64 * 18 + 256,), np.uint8)
    filled = np.ones(4097, np.uint8)
    calls = cases.abi_rejections(_lib.lib(), _lib.Catalogue, P(mask.ptr), P(labels.ptr), P(cube.ptr),
                                 P(scratch.ptr), P(counts.ptr), P(tables.ptr), _host_ptr(filled), q.handle)
    q.finish()
    wrong = [(name, got, want) for name, got, want in calls if got != want]
    assert not wrong, wrong
    assert {want for name, _, want in calls if name not in ('scratch', 'work')} == {0, cases.EINVAL, cases.EUNSUPPORTED}
    mask.assert_unchanged(q, 'mask')
    cube.assert_unchanged(q, 'cube')


def test_operator_end_to_end():
    """SmoothClip's mask of test_detect_gpu.py's finder cube is linked, filtered with min_voxels = 3 and
    measured; labels and catalogue against the twins on the mask read back; one source's own mask
    applied to the cube goes through Moments, against the same steps on the host."""
    import detect_cases
    from katsdpimager_amd import cube as cube_module, detect, link
    ctx, q = context_queue()
    data, filled, _ = detect_cases.finder_cube()
    C, P, H, W = data.shape
    frequencies = 1.4e9 + 1e5 * np.arange(C)
    the_cube = cube_module.SpectralCube(ctx, q, frequencies, P, (H, W))
    for c in np.flatnonzero(filled):
        the_cube.put(int(c), data[c], noise=1.0)
    assert np.array_equal(the_cube.filled != 0, filled != 0)
    params = detect.SmoothClipParameters(spatial_fwhm=(0, 3), spectral_widths=(1, 3, 7), threshold=3.5, border=2)
    mask = detect.SmoothClipTemplate(ctx, params).instantiate(q, data.shape)(the_cube)
    host_mask = mask.get(q)
    cases.assert_same_bits(host_mask, detect.smooth_clip_host(data, filled, params))

    link_params = link.LinkParameters(radius_xy=1.5, radius_z=1, min_voxels=3)
    assert link_params.reach_xy_sq == 2
    op = link.LinkTemplate(ctx, link_params).instantiate(q, data.shape)
    labels, catalogue = op(mask, the_cube)
    want_labels, N0 = link.link_host(host_mask, filled, 2, 1)
    table = link.measure_host(want_labels, data, filled)
    want_labels, table = link.filter_host(want_labels, table, min_voxels=3)
    assert 0 < len(table) < N0
    assert isinstance(labels, link.LabelCube) and labels.shape == data.shape
    cases.assert_same_bits(labels.get(q), want_labels)
    want = link.catalogue_host(table, data.shape, frequencies)
    assert catalogue.dtype == link.CATALOGUE_DTYPE and len(catalogue) == len(want)
    sums = _fsum_rows(want_labels, data, filled, len(table))
    for name in catalogue.dtype.names:
        if name in ('sum', 'centroid', 'frequency'):
            continue
        cases.assert_same_bits(np.ascontiguousarray(catalogue[name]), np.ascontiguousarray(want[name]), name)
    for s in range(len(table)):
        exact_sum, magnitude = sums[s][0]
        assert abs(catalogue['sum'][s] - exact_sum) <= int(table['finite'][s]) * 2.0 ** -53 * magnitude, s
    # (the centroid is a quotient of two such sums; the sources here are positive, so it is well conditioned)
    np.testing.assert_allclose(catalogue['centroid'], want['centroid'], rtol=1e-12, atol=0)
    np.testing.assert_allclose(catalogue['frequency'], want['frequency'], rtol=1e-14, atol=0)
    # again: the operator carries nothing over
    labels2, catalogue2 = op(mask, the_cube)
    cases.assert_same_bits(labels2.get(q), want_labels)
    assert len(catalogue2) == len(want)

    every = labels.mask()
    assert isinstance(every, detect.MaskCube)
    cases.assert_same_bits(every.get(q), link.label_mask_host(want_labels))
    k = int(np.argmax(table['voxels'])) + 1
    own = labels.mask(source=k)
    cases.assert_same_bits(own.get(q), link.label_mask_host(want_labels, k))
    moment_params = cube_module.MomentParameters(moments=(0,), axis='frequency')
    moments = cube_module.MomentsTemplate(ctx, moment_params).instantiate(q, data.shape)
    got = moments(own.apply(the_cube))
    host_cube = the_cube.get()
    want_cube = detect.apply_host(host_cube, link.label_mask_host(want_labels, k), the_cube.filled)
    want_maps = cube_module.moments_host(want_cube, frequencies, moment_params.cut_table(C), the_cube.filled,
                                         moment_params)
    cases.assert_same_bits(got[0].get(q), want_maps[0], 'moment 0 of one source')
    cases.assert_same_bits(got['count'].get(q), want_maps['count'], 'count of one source')
    assert (want_maps['count'] > 0).sum() == (want_labels == k).any(axis=0).sum()
