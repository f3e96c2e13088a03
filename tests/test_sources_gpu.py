"""Source spectra and line parameters on the device (csrc/cube_sources.hip) against the numpy twins
(sources.py, tested on their own in test_sources_host.py): the two entries through the C ABI inside
buffers of sentinels -- the counts by bits, the sums equal on integer cubes and within finite * 2^-53 *
sum |term| of math.fsum on Gaussian ones, the lines by bits against the twin fed the device's own spectra
-- then the operator end to end, and one band of 4096 channels.

Shapes, layouts and masks are test_link_gpu.py's: a workgroup of the spectra launch holds 1024 elements
of one channel and a wave 256, so (1, 5, 257) and (3, 33, 65) span several of both in one channel, with
16-byte and single-element loads and a tail shorter than four."""
import ctypes
import math

import numpy as np
import pytest

import link_cases
import sources_cases as cases
from helpers import context_queue

pytestmark = pytest.mark.gpu

CHANNELS = (1, 2, 3, 9, 33)
PLANES = ((1, 1, 1), (1, 3, 5), (2, 7, 9), (1, 5, 257), (3, 33, 65))
DENSITIES = (0.01, 0.1, 0.45)
_Padded = link_cases.Padded


def _device(ctx, q, host):
    from katsdpimager_amd import accel
    array = accel.DeviceArray(ctx, host.shape, host.dtype)
    array.set(q, host)
    return array


def _channel_tables(C, seed):
    """(unit, width, coord, variance): positive units and widths, descending coordinates, one channel
    without a noise."""
    rng = np.random.default_rng(seed)
    unit = 1.0 / rng.uniform(20.0, 40.0, C)
    width = rng.uniform(3.0, 5.0, C)
    coord = 1500.0 - np.cumsum(width)
    variance = rng.uniform(0.5, 2.0, C) * 1e-6
    if C > 4:
        variance[C // 3] = np.nan
    return unit, width, coord, variance


def run_case(ctx, q, labels, cube, filled, c0, offsets, layouts, exact, where=None, extra=3):
    """Both entries on one case in every layout of `layouts` against the twins; returns the device's
    (sum, voxels, finite) of the last layout."""
    from katsdpimager_amd import sources, _lib
    lib = _lib.lib()
    C = labels.shape[0]
    M = int(np.prod(labels.shape[1:]))
    N = len(c0)
    total = int(offsets[-1])
    filled = np.ascontiguousarray(filled, np.uint8)
    want = sources.source_spectra_host(labels, cube, filled, c0, offsets)
    restated = cases.restate_spectra(labels, cube, filled, c0, offsets)
    cases.assert_spectra(want, labels, cube, filled, c0, offsets, exact, (where, 'the twin'), restated)
    tables = _channel_tables(C, C)
    device_c0 = _device(ctx, q, np.concatenate((c0, np.full(1, 7, np.int32))))
    device_offsets = _device(ctx, q, offsets)
    space = _Padded(ctx, q, 1, 4 * C, None, extra, 1, np.float64)
    got = None
    for k, ((fpad, foff), _, (lpad, loff)) in enumerate(layouts):
        at = (where, labels.shape, (fpad, foff), (lpad, loff))
        the_labels = _Padded(ctx, q, C, M, labels, lpad, loff, np.int32)
        the_cube = _Padded(ctx, q, C, M, cube, fpad, foff, np.float32)
        out = [_Padded(ctx, q, 1, total, None, extra, k % 2, dtype) for dtype in (np.float64, np.int32, np.int32)]
        _lib.check(lib.kimg_cube_source_spectra(
            the_labels.ptr, the_labels.pitch, the_cube.ptr, the_cube.pitch, C, M, cases.host_ptr(filled), N,
            device_c0.ptr, device_offsets.ptr, total, out[0].ptr, out[1].ptr, out[2].ptr, q.handle), 'spectra')
        got = tuple(t.whole.get(q)[t.offset:t.offset + total] for t in out)
        # the counts by bits, and nothing but the `total` entries written
        out[1].assert_holds(q, want[1], at + ('voxels',))
        out[2].assert_holds(q, want[2], at + ('finite',))
        if exact:
            out[0].assert_holds(q, want[0], at + ('sum',))
        else:
            out[0].assert_holds(q, got[0], at + ('beyond the sums',))
            cases.assert_spectra(got, labels, cube, filled, c0, offsets, False, at, restated)
        the_labels.assert_unchanged(q, at)
        the_cube.assert_unchanged(q, at)

        # the lines of the device's own spectra
        rows = {name: _Padded(ctx, q, 1, N, None, extra, k % 2, sources.LINE_TABLE_DTYPE[name])
                for name in sources.LINE_TABLE_DTYPE.names}
        struct = _lib.SourceLineTable(**{name: r.ptr for name, r in rows.items()})
        _lib.check(lib.kimg_source_lines(
            N, device_c0.ptr, device_offsets.ptr, total, out[0].ptr, out[2].ptr, C,
            *(cases.host_ptr(t) for t in tables), space.ptr, ctypes.byref(struct), q.handle), 'lines')
        want_rows = sources.source_lines_host(c0, offsets, got[0], got[2], tables)
        for name, r in rows.items():
            r.assert_holds(q, np.ascontiguousarray(want_rows[name]), at + ('lines', name))
        if N:
            space.assert_holds(q, np.concatenate(tables), at + ('channel tables',))
        else:
            space.assert_unchanged(q, at + ('channel tables without a source',))
        for t in out:
            t.assert_holds(q, t.whole.get(q)[t.offset:t.offset + total], at + ('spectra after lines',))
    return got


def _linked(mask, filled, reach, cube):
    """(labels, c0, offsets) of a mask, the ranges from measure_host's boxes."""
    from katsdpimager_amd import link, sources
    labels, N = link.link_host(mask, filled, *reach)
    table = link.measure_host(labels, cube, filled, N)
    c0, offsets = sources.ragged(table['c0'], table['c1'])
    return labels, c0, offsets


def _cube(shape, turn):
    """(cube, exact): integer cubes (every order of a sum is exact) and Gaussian ones alternate, NaN and
    both infinities planted in each."""
    if turn % 2:
        return link_cases.integer_cube(shape, turn), True
    return cases.plant_blanks(link_cases.gaussian_cube(shape, turn), turn), False


@pytest.mark.parametrize('C', CHANNELS)
def test_entries_against_twins(C):
    ctx, q = context_queue()
    for i, plane in enumerate(PLANES):
        turn = C + i
        shape = (C,) + plane
        mask = link_cases.random_mask(shape, 10 * C + i, DENSITIES[turn % 3], values=(1, 1, 2, 255))
        if mask.size < 4:
            mask[...] = 1
        cube, exact = _cube(shape, turn)
        filled = link_cases.filled_for(C, turn)
        reach = ((1, 1), (2, 1), (1, 0), (4, 2), (9, 3))[turn % 5]
        labels, c0, offsets = _linked(mask, filled, reach, cube)
        run_case(ctx, q, labels, cube, filled, c0, offsets, link_cases.layouts(), exact, reach)


def test_all_set():
    """One label in every lane: the combining path, every wave one atomic per table."""
    ctx, q = context_queue()
    for shape in ((3, 2, 7, 9), (2, 1, 5, 257), (9, 3, 33, 65)):
        mask = np.ones(shape, np.uint8)
        filled = np.ones(shape[0], np.uint8)
        for k in range(2):
            cube, exact = _cube(shape, k + 1)
            labels, c0, offsets = _linked(mask, filled, (1, 1), cube)
            assert len(c0) == shape[1] and offsets[-1] == shape[0] * shape[1]
            got = run_case(ctx, q, labels, cube, filled, c0, offsets, link_cases.layouts(5)[2 * k:][:2], exact)
            assert list(got[1]) == [shape[2] * shape[3]] * int(offsets[-1])


def test_checkerboard():
    """Every voxel its own source at reach (1, 0): no two neighbouring lanes hold one label."""
    ctx, q = context_queue()
    shape = (3, 1, 33, 65)
    mask = link_cases.checkerboard(shape)
    filled = np.ones(3, np.uint8)
    for k in range(2):
        cube, exact = _cube(shape, k + 1)
        labels, c0, offsets = _linked(mask, filled, (1, 0), cube)
        assert len(c0) == int(mask.sum()) == offsets[-1]
        got = run_case(ctx, q, labels, cube, filled, c0, offsets, link_cases.layouts(2), exact)
        assert set(got[1]) == {1}


def test_long_runs():
    """A serpentine and combs: runs of one label that cross wave, workgroup and row boundaries, and
    that end and begin inside a thread's four elements."""
    ctx, q = context_queue()
    mask = link_cases.serpentine(33, 33, 65)
    filled = np.ones(33, np.uint8)
    cube, exact = _cube(mask.shape, 1)
    for reach, count in (((1, 1), 1), ((1, 0), 33)):
        labels, c0, offsets = _linked(mask, filled, reach, cube)
        assert len(c0) == count
        run_case(ctx, q, labels, cube, filled, c0, offsets, link_cases.layouts(2), exact, reach)
    for turn, shape in enumerate(((9, 2, 7, 9), (33, 1, 5, 257))):
        mask = link_cases.combs(shape[0], shape[1:])
        cube, exact = _cube(shape, turn)
        labels, c0, offsets = _linked(mask, np.ones(shape[0], np.uint8), (1, 1), cube)
        assert len(c0) == shape[1]
        run_case(ctx, q, labels, cube, np.ones(shape[0], np.uint8), c0, offsets, link_cases.layouts(2), exact)


def test_unfilled_channels_inside_a_range():
    """reach_z = 3 links across unfilled channels: their entries read 0 / 0 / 0."""
    ctx, q = context_queue()
    shape = (9, 1, 5, 257)
    mask = np.zeros(shape, np.uint8)
    mask[:, 0, 1:4, 100:180] = 1
    mask[:, 0, 4, 3] = 1
    filled = np.ones(9, np.uint8)
    filled[[3, 4, 7]] = 0
    cube, _ = _cube(shape, 1)
    cube[3] = 77.0                      # (never read)
    labels, c0, offsets = _linked(mask, filled, (1, 3), cube)
    assert list(c0) == [0, 0] and list(offsets) == [0, 9, 18]
    got = run_case(ctx, q, labels, cube, filled, c0, offsets, link_cases.layouts(3), True)
    for at in (3, 4, 7, 12, 13, 16):
        assert (got[0][at], got[1][at], got[2][at]) == (0.0, 0, 0), at
    assert got[1][0] == 240 and got[1][9] == 1


def test_tables_that_exclude_voxels():
    """Labels above N, a row that starts late and a row that is short: those voxels are skipped, and
    nothing but the `total` entries is written."""
    ctx, q = context_queue()
    shape = (9, 2, 7, 9)
    mask = link_cases.random_mask(shape, 5, 0.45)
    filled = link_cases.filled_for(9, 1)            # (the middle channel unfilled: six sources)
    cube, _ = _cube(shape, 1)
    labels, c0, offsets = _linked(mask, filled, (1, 1), cube)
    N = len(c0)
    assert N > 3
    fewer_c0, fewer = c0[:N - 2].copy(), offsets[:N - 1].copy()
    late, short = np.flatnonzero(np.diff(fewer) > 2)[:2]
    fewer_c0[late] += 1
    lengths = np.diff(fewer)
    lengths[short] -= 1
    fewer[1:] = np.cumsum(lengths)
    got = run_case(ctx, q, labels, cube, filled, fewer_c0, fewer, link_cases.layouts(3), True)
    assert got[1].sum() < ((labels > 0) & (filled.reshape(-1, 1, 1, 1) != 0)).sum()
    # labels that are negative are skipped too
    negative = np.where(labels == 1, -1, labels).astype(np.int32)
    got = run_case(ctx, q, negative, cube, filled, c0, offsets, link_cases.layouts(1), True)
    assert not got[1][offsets[0]:offsets[1]].any()


def test_abi_rejections():
    from katsdpimager_amd import accel, _lib
    ctx, q = context_queue()
    P = ctypes.c_void_p
    cube = _Padded(ctx, q, 4, 16, link_cases.integer_cube((4, 16), 1), 0, 0, np.float32)
    labels = _Padded(ctx, q, 4, 16, (np.arange(64) % 3).astype(np.int32), 0, 0, np.int32)
    layout = _device(ctx, q, np.array([0, 1, 0, 2, 4], np.int32))
    tables = accel.DeviceArray(ctx, (320 + 64 * 12,), np.uint8)
    filled = np.ones(4097, np.uint8)
    channel = np.ones(4097, np.float64)
    calls = cases.abi_rejections(_lib.lib(), _lib.SourceLineTable, P(labels.ptr), P(cube.ptr), P(layout.ptr),
                                 P(tables.ptr), cases.host_ptr(filled), cases.host_ptr(channel), q.handle)
    q.finish()
    wrong = [(name, got, want) for name, got, want in calls if got != want]
    assert not wrong, wrong
    assert {want for _, _, want in calls} == {0, cases.EINVAL, cases.EUNSUPPORTED}
    labels.assert_unchanged(q, 'labels')
    cube.assert_unchanged(q, 'cube')


def test_operator_end_to_end():
    """SmoothClip's mask of the finder cube, linked with min_voxels = 3, then parameterised: spectra and
    lines against the twins, twice; the spectrum of the largest source against moment 0 of its own mask
    applied to the cube, summed per channel on the host."""
    import detect_cases
    from katsdpimager_amd import beam, cube as cube_module, detect, link, sources
    ctx, q = context_queue()
    data, filled, _ = detect_cases.finder_cube()
    C, P, H, W = data.shape
    frequencies = 1.4e9 + 1e5 * np.arange(C)
    rest = 1.42040575e9
    the_cube = cube_module.SpectralCube(ctx, q, frequencies, P, (H, W))
    for c in np.flatnonzero(filled):
        the_cube.put(int(c), data[c], noise=1.0, beam=beam.Beam(1.0, 2.0 * frequencies[0] / frequencies[c], 1.5, 0.2))
    params = detect.SmoothClipParameters(spatial_fwhm=(0, 3), spectral_widths=(1, 3, 7), threshold=3.5, border=2)
    mask = detect.SmoothClipTemplate(ctx, params).instantiate(q, data.shape)(the_cube)
    linker = link.LinkTemplate(ctx, link.LinkParameters(radius_xy=1.5, radius_z=1, min_voxels=3)).instantiate(
        q, data.shape)
    labels, catalogue = linker(mask, the_cube)
    host_labels = labels.get(q)
    N = len(catalogue)
    assert N > 1

    source_params = sources.SourceParameters(rest_frequency=rest)
    op = sources.SourcesTemplate(ctx, source_params).instantiate(q, data.shape)
    tables = sources.line_tables(the_cube, 'velocity', rest)
    for again in range(2):
        spectra, lines = op(labels, the_cube, catalogue)
        assert isinstance(spectra, sources.SourceSpectra) and len(spectra) == N
        assert lines.dtype == sources.LINES_DTYPE and len(lines) == N
        assert np.array_equal(lines['id'], catalogue['id'])
        assert np.array_equal(spectra.c0, catalogue['c0'])
        assert np.array_equal(np.diff(spectra.offsets), catalogue['c1'] - catalogue['c0'] + 1)
        got = spectra.get(q)
        cases.assert_spectra(got, host_labels, data, filled, spectra.c0, spectra.offsets, False, again)
        # (the catalogue's own counts: every voxel of a source lies in its range)
        for s in range(N):
            a, b = spectra.offsets[s], spectra.offsets[s + 1]
            assert got[1][a:b].sum() == catalogue['voxels'][s] and got[2][a:b].sum() == catalogue['finite'][s]
        want = sources.source_lines_host(spectra.c0, spectra.offsets, got[0], got[2], tables)
        for name in want.dtype.names:
            link_cases.assert_same_bits(np.ascontiguousarray(lines[name]), np.ascontiguousarray(want[name]),
                                        (again, name))
        assert np.all(lines['flux_err'] > 0) and np.all(lines['channels'] == np.diff(spectra.offsets))

    # the largest source: its spectrum against the three passes this operator replaces
    k = int(np.argmax(catalogue['voxels'])) + 1
    channels, total_sum, voxels, finite = spectra.spectrum(k)
    assert list(channels) == list(range(catalogue['c0'][k - 1], catalogue['c1'][k - 1] + 1))
    own = labels.mask(source=k).apply(the_cube)
    masked = own.get()
    for c, got_sum, n in zip(channels, total_sum, finite):
        if not filled[c]:
            assert (got_sum, n) == (0.0, 0)
            continue
        terms = masked[c][np.isfinite(masked[c])].astype(np.float64)
        assert len(terms) == n
        assert abs(got_sum - math.fsum(terms)) <= n * 2.0 ** -53 * math.fsum(np.abs(terms)), c

    # an empty catalogue: empty results, no launch
    spectra, lines = op(labels, the_cube, catalogue[:0])
    assert len(spectra) == 0 and len(lines) == 0 and spectra.total == 0
    assert [len(t) for t in spectra.get(q)] == [0, 0, 0]
    # plain arrays
    spectra, lines2 = op(labels, the_cube.array, catalogue, filled=the_cube.filled, tables=tables)
    got2 = spectra.get(q)
    link_cases.assert_same_bits(got2[1], got[1])
    with pytest.raises(ValueError):
        op(labels, the_cube.array, catalogue, filled=the_cube.filled)
    with pytest.raises(ValueError):
        op(labels, the_cube, catalogue, tables=tables)


def test_a_band_of_4096_channels():
    """The ragged offsets and the channel loops at the limit: a source that spans the whole band across
    its unfilled channels (reach_z = 3), one of 2000 channels and many of a few."""
    ctx, q = context_queue()
    C, plane = 4096, (1, 3, 5)
    shape = (C,) + plane
    rng = np.random.default_rng(4096)
    mask = np.zeros(shape, np.uint8)
    mask[:, 0, 0, 0] = 1                                    # one column through the whole band
    mask[:, 0, 2, 1:5] = rng.random((C, 4)) < 0.03          # short pieces
    mask[1000:3000, 0, 0, 3:5] = 1
    filled = np.ones(C, np.uint8)
    filled[[0, 31, 32, 2047, 2048, 3000, 4095]] = 0
    cube, exact = _cube(shape, 1)
    labels, c0, offsets = _linked(mask, filled, (1, 3), cube)
    lengths = np.diff(offsets)
    assert len(c0) > 100 and lengths.max() == 4094 and (lengths == 2000).any() and offsets[-1] > C + 2000
    got = run_case(ctx, q, labels, cube, filled, c0, offsets, link_cases.layouts(2), exact)
    assert got[1].sum() == (mask[filled != 0] != 0).sum()
