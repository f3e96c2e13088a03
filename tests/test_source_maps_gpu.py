"""Per-source moment maps on the device (csrc/cube_source_maps.hip) against the numpy twin
(source_maps.source_maps_host, tested on its own in test_source_maps_host.py): the two entries through
the C ABI inside buffers of sentinels, every output table by bits and nothing but its `total` entries
written, labels and cube unchanged -- then the operator end to end against the three passes it replaces,
and one band of 4096 channels.

A workgroup holds 256 threads of four consecutive plane elements: the planes (1, 5, 257) and (3, 33, 65)
span several waves and workgroups, rows that a thread's four elements straddle, the 16-byte and the
single-element form (link_cases.layouts) and a tail shorter than four."""
import ctypes

import numpy as np
import pytest

import link_cases
import source_maps_cases as cases
import sources_cases
from helpers import context_queue

pytestmark = pytest.mark.gpu

CHANNELS = (1, 2, 3, 9, 33)
PLANES = ((1, 1, 1), (1, 3, 5), (2, 7, 9), (1, 5, 257), (3, 33, 65))
DENSITIES = (0.01, 0.1, 0.45)
REACHES = ((1, 1), (2, 1), (1, 0), (9, 3))
BITS = {0: 1, 1: 2, 2: 4, 8: 8, 9: 16, 'count': 32}
_Padded = link_cases.Padded


def _device(ctx, q, host):
    from katsdpimager_amd import accel
    array = accel.DeviceArray(ctx, host.shape, host.dtype)
    array.set(q, host)
    return array


def _cube(shape, seed):
    return sources_cases.plant_blanks(link_cases.gaussian_cube(shape, seed), seed)


def _dtype(key):
    return np.int32 if key == 'count' else np.float32


def _aligned(M):
    """Two layouts in which labels, cube and both pitches are 16-byte aligned -- the four-element form,
    which link_cases.layouts() never gives on planes whose size is no multiple of four -- at offsets of 0
    and 16 bytes."""
    pad = -M % 4
    return [((pad, 0), None, (pad, 0)), ((pad + 4, 4), None, (pad, 4))]


def run_case(ctx, q, labels, cube, filled, rows, total, x, layouts, where=None, extra=3):
    """Both entries on one case in every layout of `layouts` and of _aligned() against the twin; returns
    the twin's tables."""
    from katsdpimager_amd import source_maps, _lib
    lib = _lib.lib()
    C, P, H, W = labels.shape
    M = P * H * W
    N = len(rows)
    filled = np.ascontiguousarray(filled, np.uint8)
    want = source_maps.source_maps_host(labels, cube, filled, rows, total, x)
    device_x = _device(ctx, q, np.ascontiguousarray(x, np.float64))
    # (a row more than there are: a device pointer even without a source)
    device_rows = _device(ctx, q, np.concatenate((rows, np.zeros(1, source_maps.ROW_DTYPE))).view(np.uint8))
    state_bytes = 36 * total
    assert lib.kimg_cube_source_maps_workspace_bytes(total) == state_bytes
    words = (state_bytes + 7) // 8
    for k, ((fpad, foff), _, (lpad, loff)) in enumerate(list(layouts) + _aligned(M)):
        at = (where, labels.shape, (fpad, foff), (lpad, loff))
        the_labels = _Padded(ctx, q, C, M, labels, lpad, loff, np.int32)
        the_cube = _Padded(ctx, q, C, M, cube, fpad, foff, np.float32)
        state = _Padded(ctx, q, 1, words, None, extra, k % 2, np.float64)
        out = {key: _Padded(ctx, q, 1, total, None, extra, k % 2, _dtype(key)) for key in cases.KEYS}
        # every table on even turns, two of them on odd ones: what is not asked for is not written
        asked = cases.KEYS if k % 2 == 0 else (1, 'count')
        outputs = sum(BITS[key] for key in asked)
        _lib.check(lib.kimg_cube_source_maps(
            the_labels.ptr, the_labels.pitch, the_cube.ptr, the_cube.pitch, C, P, H, W, cases.host_ptr(filled),
            device_x.ptr, N, device_rows.ptr, total, state.ptr, state_bytes, q.handle), 'maps')
        _lib.check(lib.kimg_source_maps_finish(
            N, device_rows.ptr, total, state.ptr, state_bytes, device_x.ptr, C, outputs,
            *(out[key].ptr for key in cases.KEYS), q.handle), 'finish')
        for key in cases.KEYS:
            if key in asked and N and total:
                out[key].assert_holds(q, want[key], at + (key,))
            else:
                out[key].assert_unchanged(q, at + (key, 'not asked for'))
        # the state: nothing before it and nothing behind its last word
        got_state, clean = state.whole.get(q), state.host
        assert np.array_equal(got_state[:state.offset].view(np.uint8), clean[:state.offset].view(np.uint8)), at
        assert np.array_equal(got_state[state.offset + words:].view(np.uint8),
                              clean[state.offset + words:].view(np.uint8)), at
        the_labels.assert_unchanged(q, at)
        the_cube.assert_unchanged(q, at)
    return want


@pytest.mark.parametrize('C', CHANNELS)
def test_entries_against_twin(C):
    ctx, q = context_queue()
    x = cases.coordinates(C)
    for i, plane in enumerate(PLANES):
        turn = C + i
        shape = (C,) + plane
        mask = link_cases.random_mask(shape, 10 * C + i, DENSITIES[turn % 3], values=(1, 1, 2, 255))
        if mask.size < 4:
            mask[...] = 1
        cube = _cube(shape, turn)
        filled = link_cases.filled_for(C, turn)
        reach = REACHES[turn % 4]
        labels, rows, total = cases.linked(mask, filled, reach, cube, x)
        want = run_case(ctx, q, labels, cube, filled, rows, total, x, link_cases.layouts(), reach)
        assert want['count'].sum() == ((labels > 0) & np.isfinite(cube) & (filled.reshape(-1, 1, 1, 1) != 0)).sum()


def test_all_set():
    """One label in every lane and no label change at all: a source per polarization."""
    ctx, q = context_queue()
    for turn, shape in enumerate(((3, 2, 7, 9), (2, 1, 5, 257), (9, 3, 33, 65))):
        mask = np.ones(shape, np.uint8)
        filled = np.ones(shape[0], np.uint8)
        x = cases.coordinates(shape[0])
        cube = _cube(shape, turn)
        labels, rows, total = cases.linked(mask, filled, (1, 1), cube, x)
        assert len(rows) == shape[1] and total == shape[1] * shape[2] * shape[3]
        want = run_case(ctx, q, labels, cube, filled, rows, total, x, link_cases.layouts(5)[turn:][:3])
        assert np.array_equal(want['count'], np.isfinite(cube).sum(axis=0).reshape(-1))


def test_checkerboard():
    """Every voxel its own source with a box of one pixel at reach (1, 0): a label change at every
    voxel of a pixel, each to a source that is never met again."""
    ctx, q = context_queue()
    shape = (3, 1, 33, 65)
    mask = link_cases.checkerboard(shape)
    filled = np.ones(3, np.uint8)
    x = cases.coordinates(3)
    cube = _cube(shape, 1)
    labels, rows, total = cases.linked(mask, filled, (1, 0), cube, x)
    assert len(rows) == int(mask.sum()) == total
    want = run_case(ctx, q, labels, cube, filled, rows, total, x, link_cases.layouts(2))
    assert set(want['count']) == {0, 1}


def test_long_runs():
    """A serpentine and combs: boxes as large as the plane around sources that touch few of its pixels,
    and runs of one label that end and begin inside a thread's four elements."""
    ctx, q = context_queue()
    mask = link_cases.serpentine(33, 33, 65)
    filled = np.ones(33, np.uint8)
    x = cases.coordinates(33)
    cube = _cube(mask.shape, 1)
    for reach, count in (((1, 1), 1), ((1, 0), 33)):
        labels, rows, total = cases.linked(mask, filled, reach, cube, x)
        assert len(rows) == count
        run_case(ctx, q, labels, cube, filled, rows, total, x, link_cases.layouts(2), reach)
    for turn, shape in enumerate(((9, 2, 7, 9), (33, 1, 5, 257))):
        mask = link_cases.combs(shape[0], shape[1:])
        x = cases.coordinates(shape[0])
        cube = _cube(shape, turn)
        labels, rows, total = cases.linked(mask, np.ones(shape[0], np.uint8), (1, 1), cube, x)
        assert len(rows) == shape[1]
        run_case(ctx, q, labels, cube, np.ones(shape[0], np.uint8), rows, total, x, link_cases.layouts(2))


@pytest.mark.parametrize('shape, N', (((9, 2, 7, 9), 5), ((33, 1, 5, 257), 6), ((9, 3, 33, 65), 7)))
def test_sources_left_and_resumed(shape, N):
    """Hand-made labels drawn per voxel from 0 .. N, every box the whole plane: every pixel leaves and
    resumes several sources along the channel axis -- the store and the load at nearly every step -- and
    every sum still has the twin's order.  Checked once more against the restatement, on the smallest."""
    ctx, q = context_queue()
    C = shape[0]
    x = cases.coordinates(C)
    cube = _cube(shape, N)
    filled = link_cases.filled_for(C, 1)
    labels = cases.random_labels(shape, N, N)
    rows, total = cases.whole_plane_rows(shape, N, x)
    want = run_case(ctx, q, labels, cube, filled, rows, total, x, link_cases.layouts(4))
    assert want['count'].max() > 1
    if N == 5:
        cases.assert_tables(want, cases.restate(labels, cube, filled, rows, total, x), 'the restatement')


def test_unfilled_channels_inside_a_range():
    """reach_z = 3 links across unfilled channels: they are not read, and the sums go on behind them."""
    ctx, q = context_queue()
    shape = (9, 1, 5, 257)
    mask = np.zeros(shape, np.uint8)
    mask[:, 0, 1:4, 100:180] = 1
    mask[:, 0, 4, 3] = 1
    filled = np.ones(9, np.uint8)
    filled[[3, 4, 7]] = 0
    x = cases.coordinates(9)
    cube = link_cases.integer_cube(shape, 1)
    cube[3] = 5000.0                    # (never read)
    labels, rows, total = cases.linked(mask, filled, (1, 3), cube, x)
    assert list(rows['c0']) == [0, 0] and list(rows['c1']) == [8, 8] and total == 3 * 80 + 1
    want = run_case(ctx, q, labels, cube, filled, rows, total, x, link_cases.layouts(3))
    assert want['count'].max() <= 6 and not np.any(want[8] == 5000.0)
    cases.assert_tables(want, cases.restate(labels, cube, filled, rows, total, x), 'the restatement')


def _columns(rows, source, c0=0, c1=0):
    first, last = rows['c0'].copy(), rows['c1'].copy()
    first[source] += c0
    last[source] += c1
    return (rows['pol'], rows['y0'], rows['y0'] + rows['h'] - 1, rows['x0'], rows['x0'] + rows['w'] - 1,
            first, last)


def test_tables_that_exclude_voxels():
    """Labels above N and below 0, a box narrowed by a row and a column, a range c0 + 1 .. c1 - 1, a wrong
    polarization and a total cut short: the excluded voxels are skipped, and nothing outside the tables
    is written."""
    from katsdpimager_amd import source_maps
    ctx, q = context_queue()
    shape = (9, 2, 7, 9)
    mask = link_cases.random_mask(shape, 5, 0.45)
    filled = link_cases.filled_for(9, 1)
    cube = _cube(shape, 1)
    x = cases.coordinates(9)
    labels, rows, total = cases.linked(mask, filled, (1, 1), cube, x)
    N = len(rows)
    assert N > 3
    layouts = link_cases.layouts(3)
    full = run_case(ctx, q, labels, cube, filled, rows, total, x, layouts, 'as measured')
    fewer = run_case(ctx, q, labels, cube, filled, rows[:N - 2], int(rows['offset'][N - 2]), x, layouts,
                     'labels above N')
    assert fewer['count'].sum() < full['count'].sum()
    negative = np.where(labels == 1, -1, labels).astype(np.int32)
    got = run_case(ctx, q, negative, cube, filled, rows, total, x, layouts[:1], 'negative labels')
    assert not got['count'][:rows['offset'][1]].any()
    big = int(np.argmax(rows['h'] * rows['w']))
    assert rows['h'][big] > 2 and rows['w'][big] > 2 and rows['c1'][big] - rows['c0'][big] > 2
    narrow = rows.copy()
    narrow['h'][big] -= 1
    narrow['w'][big] -= 1
    got = run_case(ctx, q, labels, cube, filled, narrow, total, x, layouts, 'a narrowed box')
    assert got['count'].sum() < full['count'].sum()
    inner = source_maps.source_rows(*_columns(rows, big, c0=1, c1=-1), x, cases.CHANNEL_WIDTH)[0]
    got = run_case(ctx, q, labels, cube, filled, inner, total, x, layouts, 'a narrowed range')
    assert got['count'].sum() < full['count'].sum()
    other = rows.copy()
    other['pol'][big] = 1 - other['pol'][big]
    got = run_case(ctx, q, labels, cube, filled, other, total, x, layouts, 'a wrong polarization')
    a, b = int(rows['offset'][big]), int(rows['offset'][big] + rows['h'][big] * rows['w'][big])
    assert not got['count'][a:b].any()
    short = run_case(ctx, q, labels, cube, filled, rows, total - 5, x, layouts, 'a total cut short')
    cases.assert_tables(short, {key: table[:total - 5] for key, table in full.items()}, 'the entries kept')


def test_abi_rejections():
    from katsdpimager_amd import accel, source_maps, _lib
    ctx, q = context_queue()
    P = ctypes.c_void_p
    cube = _Padded(ctx, q, 4, 16, link_cases.integer_cube((4, 16), 1), 0, 0, np.float32)
    labels = _Padded(ctx, q, 4, 16, (np.arange(64) % 3).astype(np.int32), 0, 0, np.int32)
    x = cases.coordinates(4)
    zero, one = np.zeros(2, np.int64), np.ones(2, np.int64)
    rows, total = source_maps.source_rows(zero, 2 * np.arange(2), 2 * np.arange(2) + 1, one, one + 1, zero, zero + 3,
                                          x)
    assert total == 8
    device_x = _device(ctx, q, x)
    device_rows = _device(ctx, q, rows.view(np.uint8))
    state = accel.DeviceArray(ctx, (36,), np.float64)
    out = accel.DeviceArray(ctx, (6 * 64,), np.uint8)
    filled = np.ones(4097, np.uint8)
    calls = cases.abi_rejections(_lib.lib(), P(labels.ptr), P(cube.ptr), P(device_x.ptr), P(device_rows.ptr),
                                 P(state.ptr), P(out.ptr), cases.host_ptr(filled), q.handle)
    q.finish()
    wrong = [(name, got, want) for name, got, want in calls if got != want]
    assert not wrong, wrong
    assert {want for name, _, want in calls if name != 'bytes'} == {0, cases.EINVAL, cases.EUNSUPPORTED,
                                                                     cases.EWORKSPACE}
    labels.assert_unchanged(q, 'labels')
    cube.assert_unchanged(q, 'cube')


def test_a_band_of_4096_channels():
    """The channel loop and the per-channel bits at the limit, with the mask of
    test_sources_gpu.test_a_band_of_4096_channels: a source through the whole band across its unfilled
    channels, one of 2000 channels and many of a few."""
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
    x = cases.coordinates(C)
    cube = _cube(shape, 1)
    labels, rows, total = cases.linked(mask, filled, (1, 3), cube, x)
    lengths = rows['c1'] - rows['c0'] + 1
    assert len(rows) > 100 and lengths.max() == 4094 and (lengths == 2000).any()
    want = run_case(ctx, q, labels, cube, filled, rows, total, x, link_cases.layouts(2))
    # the column through the whole band is source 1, a box of one pixel: its finite voxels in filled channels
    assert rows['h'][0] * rows['w'][0] == 1
    assert want['count'][0] == np.isfinite(cube[filled != 0, 0, 0, 0]).sum() > 3000


def test_operator_end_to_end():
    """SmoothClip's mask of the finder cube, linked with min_voxels = 3, then mapped, twice: the maps of
    the largest source and two others against the box cut from cube.Moments over (c0, c1 + 1) of
    labels.mask(source=k) applied to the cube -- the three passes per source that this replaces."""
    import detect_cases
    from katsdpimager_amd import beam, cube as cube_module, detect, link, source_maps
    ctx, q = context_queue()
    data, filled, _ = detect_cases.finder_cube()
    C, P, H, W = data.shape
    frequencies = 1.4e9 + 1e5 * np.arange(C)
    rest = 1.42040575e9
    the_cube = cube_module.SpectralCube(ctx, q, frequencies, P, (H, W), channel_width=1e5)
    for c in np.flatnonzero(filled):
        the_cube.put(int(c), data[c], noise=1.0, beam=beam.Beam(1.0, 2.0 * frequencies[0] / frequencies[c], 1.5, 0.2))
    params = detect.SmoothClipParameters(spatial_fwhm=(0, 3), spectral_widths=(1, 3, 7), threshold=3.5, border=2)
    mask = detect.SmoothClipTemplate(ctx, params).instantiate(q, data.shape)(the_cube)
    linker = link.LinkTemplate(ctx, link.LinkParameters(radius_xy=1.5, radius_z=1, min_voxels=3)).instantiate(
        q, data.shape)
    labels, catalogue = linker(mask, the_cube)
    host_labels = labels.get(q)
    N = len(catalogue)
    assert N > 3

    moments = (0, 1, 2, 8, 9)
    map_params = source_maps.SourceMapParameters(moments=moments, rest_frequency=rest)
    op = source_maps.SourceMapsTemplate(ctx, map_params).instantiate(q, data.shape)
    x = the_cube.coordinates('velocity', rest)
    rows, total = source_maps.source_rows(*(catalogue[n] for n in ('polarization', 'y0', 'y1', 'x0', 'x1', 'c0', 'c1')),
                                          x, the_cube.axis_channel_width('velocity', rest))
    want = source_maps.source_maps_host(host_labels, data, filled, rows, total, x)
    largest = int(np.argmax(catalogue['voxels'])) + 1
    chosen = [largest] + [k for k in (1, N) if k != largest][:2]
    if len(chosen) < 3:
        chosen.append(2 if 2 not in chosen else 3)
    for again in range(2):
        maps = op(labels, the_cube, catalogue)
        assert isinstance(maps, source_maps.SourceMaps) and len(maps) == N and maps.total == total
        assert maps.ready is not None and np.array_equal(maps.rows, rows)
        cases.assert_tables(maps.get(q), want, again)
    for k in chosen:
        row = catalogue[k - 1]
        c0, c1 = int(row['c0']), int(row['c1'])
        assert maps.origin(k) == (row['polarization'], row['y0'], row['x0'])
        own = labels.mask(source=k).apply(the_cube)
        three = cube_module.MomentsTemplate(ctx, cube_module.MomentParameters(
            moments=moments, rest_frequency=rest, channels=(c0, c1 + 1))).instantiate(q, data.shape)(own)
        got = maps.map(k)
        assert set(got) == set(cases.KEYS)
        for key in cases.KEYS:
            box = three[key].get(q)[row['polarization'], row['y0']:row['y1'] + 1, row['x0']:row['x1'] + 1]
            link_cases.assert_same_bits(got[key], np.ascontiguousarray(box), (k, key))
        assert got['count'].sum() == row['finite'] and got['count'].shape == (row['y1'] - row['y0'] + 1,
                                                                             row['x1'] - row['x0'] + 1)
    with pytest.raises(ValueError):
        maps.map(0)
    with pytest.raises(ValueError):
        maps.origin(N + 1)

    # an empty catalogue: an empty result, no launch
    empty = op(labels, the_cube, catalogue[:0])
    assert len(empty) == 0 and empty.total == 0 and empty.ready is None
    assert {key: len(table) for key, table in empty.get(q).items()} == dict.fromkeys(cases.KEYS, 0)
    # plain arrays
    plain = op(labels, the_cube.array, catalogue, filled=the_cube.filled, frequencies=frequencies,
               channel_width=1e5)
    cases.assert_tables(plain.get(q), want, 'plain arrays')
    with pytest.raises(ValueError):
        op(labels, the_cube.array, catalogue, filled=the_cube.filled)
    with pytest.raises(ValueError):
        op(labels, the_cube, catalogue, frequencies=frequencies)
    with pytest.raises(ValueError):
        op(labels, the_cube, catalogue[['id', 'c0', 'c1']])
    # the cap on the sum of box areas
    small = source_maps.SourceMapsTemplate(ctx, source_maps.SourceMapParameters(
        moments=(0,), rest_frequency=rest, max_entries=total - 1)).instantiate(q, data.shape)
    with pytest.raises(ValueError, match='{} entries.*max_entries = {}'.format(total, total - 1)):
        small(labels, the_cube, catalogue)
    fewer = small(labels, the_cube, catalogue[:N - 1])
    assert set(fewer.get(q)) == {0, 'count'}
    link_cases.assert_same_bits(fewer.get(q)[0], want[0][:fewer.total])
