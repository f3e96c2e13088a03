"""The numpy twin of the per-source moment maps (source_maps.source_maps_host) against a restatement
that shares nothing with it (source_maps_cases.restate: cube.moments_host on each source's own cube), by
bits for every moment and the count; the rows table; parameter validation; the max_entries refusal and
the empty catalogue."""
import numpy as np
import pytest

import link_cases
import source_maps_cases as cases
import sources_cases

REACHES = ((1, 1), (2, 1), (1, 0), (9, 3))


def _cube(shape, seed):
    return sources_cases.plant_blanks(link_cases.gaussian_cube(shape, seed), seed)


def _filled(C, turn):
    """Unfilled channels: the middle one on odd turns, the first one too when there are five or more."""
    filled = link_cases.filled_for(C, turn)
    if C >= 5 and turn % 2:
        filled[0] = 0
    return filled


def _check(mask, reach, turn, where):
    from katsdpimager_amd import source_maps
    shape = mask.shape
    C = shape[0]
    cube = _cube(shape, turn)
    filled = _filled(C, turn)
    x = cases.coordinates(C, turn)
    labels, rows, total = cases.linked(mask, filled, reach, cube, x)
    got = source_maps.source_maps_host(labels, cube, filled, rows, total, x)
    want = cases.restate(labels, cube, filled, rows, total, x)
    cases.assert_tables(got, want, (where, shape, reach))
    assert got['count'].sum() == ((labels > 0) & np.isfinite(cube) & (filled.reshape(-1, 1, 1, 1) != 0)).sum()
    return len(rows)


@pytest.mark.parametrize('density', (0.01, 0.1, 0.45))
def test_random_masks(density):
    for turn, (shape, reach) in enumerate(zip(((9, 2, 7, 9), (3, 1, 5, 33), (5, 3, 9, 11), (2, 1, 3, 5)), REACHES)):
        mask = link_cases.random_mask(shape, turn + int(100 * density), density, values=(1, 2, 255))
        _check(mask, reach, turn + 1, density)


def test_checkerboard():
    """Every voxel its own one-pixel box at reach (1, 0); one source per plane at (2, 1)."""
    shape = (3, 2, 7, 9)
    mask = link_cases.checkerboard(shape)
    assert _check(mask, (1, 0), 1, 'checkerboard') == int(mask.sum()) - int(mask[1].sum())
    assert _check(mask, (2, 1), 2, 'checkerboard') == 2


def test_serpentine_and_combs():
    for reach in ((1, 1), (1, 0)):
        _check(link_cases.serpentine(5, 7, 9), reach, 2, 'serpentine')
    for reach in REACHES:
        _check(link_cases.combs(5, (2, 5, 7)), reach, 3, 'combs')


def test_overlapping_boxes_and_a_source_left_and_resumed():
    """A ring around a dot: the dot's box lies inside the ring's, their entries apart.  And hand-made
    labels drawn per voxel: every pixel leaves and resumes several sources along the channel axis."""
    from katsdpimager_amd import source_maps
    mask = np.zeros((4, 1, 7, 7), np.uint8)
    mask[:, 0, 0, :] = mask[:, 0, 6, :] = mask[:, 0, :, 0] = mask[:, 0, :, 6] = 1
    mask[1:3, 0, 3, 3] = 1
    assert _check(mask, (1, 1), 0, 'ring') == 2
    shape = (9, 2, 3, 5)
    cube = _cube(shape, 5)
    x = cases.coordinates(9)
    filled = _filled(9, 1)
    labels = cases.random_labels(shape, 5, 7)
    rows, total = cases.whole_plane_rows(shape, 5, x)
    assert total == 5 * 15
    got = source_maps.source_maps_host(labels, cube, filled, rows, total, x)
    cases.assert_tables(got, cases.restate(labels, cube, filled, rows, total, x), 'random labels')


def test_tables_that_exclude_voxels():
    """Labels outside 1 .. N, a narrowed box, a narrowed range, a wrong polarization and a total cut
    short: the voxels they leave out are skipped, in the twin as in the restatement."""
    from katsdpimager_amd import source_maps
    shape = (9, 2, 7, 9)
    mask = link_cases.random_mask(shape, 5, 0.45)
    filled = link_cases.filled_for(9, 1)
    cube = _cube(shape, 1)
    x = cases.coordinates(9)
    labels, rows, total = cases.linked(mask, filled, (1, 1), cube, x)
    N = len(rows)
    assert N > 3
    full = source_maps.source_maps_host(labels, cube, filled, rows, total, x)

    def both(labels, rows, total, where):
        got = source_maps.source_maps_host(labels, cube, filled, rows, total, x)
        cases.assert_tables(got, cases.restate(labels, cube, filled, rows, total, x), where)
        return got

    fewer = both(labels, rows[:N - 2], int(rows['offset'][N - 2]), 'labels above N')
    assert fewer['count'].sum() < full['count'].sum()
    negative = np.where(labels == 1, -1, labels).astype(np.int32)
    got = both(negative, rows, total, 'negative labels')
    assert not got['count'][:rows['offset'][1]].any()
    big = int(np.argmax(rows['h'] * rows['w']))
    assert rows['h'][big] > 2 and rows['w'][big] > 2 and rows['c1'][big] - rows['c0'][big] > 2
    narrow = rows.copy()
    narrow['h'][big] -= 1
    narrow['w'][big] -= 1
    got = both(labels, narrow, total, 'a narrowed box')
    assert got['count'].sum() < full['count'].sum()
    inner = source_maps.source_rows(*_columns(rows, big, c0=1, c1=-1), x, cases.CHANNEL_WIDTH)[0]
    got = both(labels, inner, total, 'a narrowed range')
    assert got['count'].sum() < full['count'].sum()
    other = rows.copy()
    other['pol'][big] = 1 - other['pol'][big]
    got = both(labels, other, total, 'a wrong polarization')
    a, b = int(rows['offset'][big]), int(rows['offset'][big] + rows['h'][big] * rows['w'][big])
    assert not got['count'][a:b].any() and np.isnan(got[0][a:b]).all()
    short = both(labels, rows, total - 5, 'a total cut short')
    cases.assert_tables(short, {key: table[:total - 5] for key, table in full.items()}, 'the entries kept')


def test_a_band_of_4096_channels():
    """The twin at the band limit, with the mask of test_sources_gpu.test_a_band_of_4096_channels."""
    from katsdpimager_amd import source_maps
    C = 4096
    shape = (C, 1, 3, 5)
    rng = np.random.default_rng(4096)
    mask = np.zeros(shape, np.uint8)
    mask[:, 0, 0, 0] = 1
    mask[:, 0, 2, 1:5] = rng.random((C, 4)) < 0.03
    mask[1000:3000, 0, 0, 3:5] = 1
    filled = np.ones(C, np.uint8)
    filled[[0, 31, 32, 2047, 2048, 3000, 4095]] = 0
    x = cases.coordinates(C)
    cube = _cube(shape, 1)
    labels, rows, total = cases.linked(mask, filled, (1, 3), cube, x)
    assert len(rows) > 100 and (rows['c1'] - rows['c0']).max() == 4093
    got = source_maps.source_maps_host(labels, cube, filled, rows, total, x)
    cases.assert_tables(got, cases.restate(labels, cube, filled, rows, total, x), 'a band of 4096')


def _columns(rows, source, c0=0, c1=0):
    """The arguments of source_rows that give `rows`, the range of `source` moved by (c0, c1)."""
    first, last = rows['c0'].copy(), rows['c1'].copy()
    first[source] += c0
    last[source] += c1
    return (rows['pol'], rows['y0'], rows['y0'] + rows['h'] - 1, rows['x0'], rows['x0'] + rows['w'] - 1,
            first, last)


def test_source_rows():
    from katsdpimager_amd import cube, source_maps
    x = cases.coordinates(9)
    args = (np.array([0, 1, 0]), np.array([1, 0, 2]), np.array([3, 0, 2]), np.array([2, 4, 0]),
            np.array([2, 6, 5]), np.array([0, 3, 8]), np.array([8, 3, 8]))
    rows, total = source_maps.source_rows(*args, x, 1.25)
    assert rows.dtype == source_maps.ROW_DTYPE and rows.dtype.itemsize == 48
    assert list(rows['offset']) == [0, 3, 6] and total == 12
    assert list(rows['h']) == [3, 1, 1] and list(rows['w']) == [1, 3, 6]
    for s in range(3):
        c0, c1 = int(rows['c0'][s]), int(rows['c1'][s])
        assert rows['x_ref'][s] == x[(c0 + c1 + 1) // 2]
        assert rows['width'][s] == cube.range_width(x, c0, c1 + 1, 1.25)
    with pytest.raises(ValueError, match='channel width'):
        source_maps.source_rows(*args, x)
    with pytest.raises(ValueError, match='12 entries.*max_entries = 11'):
        source_maps.source_rows(*args, x, 1.25, max_entries=11)
    for k, bad in ((1, np.array([1, 0, 3])), (5, np.array([0, 4, 8])), (6, np.array([8, 3, 9])),
                   (0, np.array([0, -1, 0])), (2, np.array([3, 0]))):
        with pytest.raises(ValueError):
            source_maps.source_rows(*(bad if i == k else a for i, a in enumerate(args)), x, 1.25)
    empty = np.zeros(0, np.int32)
    rows, total = source_maps.source_rows(*([empty] * 7), x)
    assert len(rows) == 0 and total == 0


def test_twin_refuses():
    from katsdpimager_amd import source_maps
    labels = np.zeros((2, 1, 3, 3), np.int32)
    cube = np.zeros((2, 1, 3, 3), np.float32)
    x = cases.coordinates(2)
    rows, total = cases.whole_plane_rows(labels.shape, 1, x)
    good = dict(labels=labels, cube=cube, filled=np.ones(2), rows=rows, total=total, x=x)
    out = source_maps.source_maps_host(**good)
    assert set(out) == set(cases.KEYS) and not out['count'].any() and np.isnan(out[8]).all()
    assert list(source_maps.source_maps_host(outputs=('count', 1), **good)) == [1, 'count']
    for change in (dict(labels=labels.astype(np.int64)), dict(cube=cube.astype(np.float64)), dict(cube=cube[:1]),
                   dict(filled=np.ones(3)), dict(rows=rows.view(np.uint8)), dict(total=-1), dict(x=x[:1]),
                   dict(outputs=()), dict(outputs=(3,)), dict(outputs=(0, 0)), dict(outputs=(True,))):
        with pytest.raises(ValueError):
            source_maps.source_maps_host(**dict(good, **change))
    # no source at all: every entry NaN and 0
    none = source_maps.source_maps_host(labels, cube, np.ones(2), rows[:0], 4, x)
    assert not none['count'].any() and np.isnan(none[0]).all()


def test_parameters():
    from katsdpimager_amd import source_maps
    Parameters = source_maps.SourceMapParameters
    params = Parameters(rest_frequency=1.42e9)
    assert params.moments == (0, 1, 2) and params.axis == 'velocity' and params.max_entries == 2 ** 26
    assert Parameters((9, 0), 'frequency').moments == (0, 9)
    assert 'max_entries=7' in repr(Parameters((8,), 'frequency', max_entries=7))
    for args, kwargs in (((), {}),                                      # velocity without a rest frequency
                         (((),), dict(axis='frequency')), (((3,),), dict(axis='frequency')),
                         (((0, 0),), dict(axis='frequency')), (((True,),), dict(axis='frequency')),
                         ((5,), dict(axis='frequency')), (((0,), 'wavelength'), {}),
                         (((0,),), dict(rest_frequency=-1.0)), (((0,),), dict(rest_frequency=True)),
                         (((0,),), dict(rest_frequency=np.nan)),
                         (((0,), 'frequency'), dict(max_entries=0)), (((0,), 'frequency'), dict(max_entries=2 ** 31 - 1)),
                         (((0,), 'frequency'), dict(max_entries=True)), (((0,), 'frequency'), dict(max_entries=1.5))):
        with pytest.raises(ValueError):
            Parameters(*args, **kwargs)
    with pytest.raises(TypeError):
        source_maps.SourceMapsTemplate(None, object())


def test_the_module_says_what_is_left():
    from katsdpimager_amd import link, source_maps, sources
    assert 'Not done' in source_maps.__doc__ and 'pasting the maps back' in source_maps.__doc__
    for module in (link, sources):
        left = module.__doc__[module.__doc__.index('Not done'):]
        assert 'per-source moment maps' not in left
