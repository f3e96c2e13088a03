"""The numpy twins of the "Source linking" contracts (katsdpimager_amd/link.py) against a plain-Python
restatement (link_cases.restate: a flood fill over an explicit neighbour list, math.fsum for the sums),
against scipy.ndimage.label where scipy is present, and on known answers.  No GPU."""
import numpy as np
import pytest

import link_cases as cases
from katsdpimager_amd import link


def _ones(mask):
    return np.ones(mask.shape[0], np.uint8)


def _plane(rows):
    """A (1, 1, H, W) mask from strings of '#' and '.'."""
    return np.array([[c == '#' for c in row] for row in rows], np.uint8)[np.newaxis, np.newaxis]


@pytest.mark.parametrize('seed', range(4))
def test_twins_against_restatement(seed):
    shape = ((5, 2, 9, 11), (1, 1, 7, 8), (9, 1, 5, 6), (3, 3, 4, 4))[seed]
    mask = cases.random_mask(shape, seed, (0.3, 0.45, 0.15, 0.5)[seed], values=(1, 2, 255))
    filled = cases.filled_for(shape[0], seed + 1)
    for k, (reach_xy_sq, reach_z) in enumerate(cases.REACHES):
        labels, N0 = link.link_host(mask, filled, reach_xy_sq, reach_z)
        want_labels, want_N0, rows = cases.restate(mask, filled, None, reach_xy_sq, reach_z)
        assert N0 == want_N0
        cases.assert_same_bits(labels, want_labels, (reach_xy_sq, reach_z))
    for k, cube in enumerate((cases.integer_cube(shape, seed), cases.gaussian_cube(shape, seed))):
        labels, N0 = link.link_host(mask, filled, 2, 1)
        _, _, rows = cases.restate(mask, filled, cube, 2, 1)
        table = link.measure_host(labels, cube, filled)
        assert table.dtype == link.TABLE_DTYPE
        cases.assert_table(table, rows, k, exact_sums=k == 0)
        # a capacity below N0: the first rows only
        short = link.measure_host(labels, cube, filled, N0, max(N0 // 2, 1))
        cases.assert_same_bits(short, table[:max(N0 // 2, 1)])


@pytest.mark.parametrize('reach', [(1, 1), (2, 1), (1, 0)])
def test_labels_against_scipy(reach):
    ndimage = pytest.importorskip('scipy.ndimage')
    mask = cases.random_mask((6, 2, 17, 19), 11, 0.35)
    filled = np.array([1, 1, 1, 0, 1, 1], np.uint8)
    structure = np.zeros((3, 3, 3, 3), bool)
    structure[1 - reach[1]:2 + reach[1], 1] = ndimage.generate_binary_structure(2, reach[0])
    want, count = ndimage.label((mask != 0) & (filled.reshape(-1, 1, 1, 1) != 0), structure)
    labels, N0 = link.link_host(mask, filled, *reach)
    assert N0 == count
    assert np.array_equal(labels, want)


def test_diagonal_pair():
    mask = _plane(['#.', '.#'])
    assert link.link_host(mask, [1], 1, 0)[1] == 2
    assert link.link_host(mask, [1], 2, 0)[1] == 1
    assert link.link_host(mask, [1], 0, 0)[1] == 2


def test_gaps_in_the_plane_and_along_the_channels():
    one, two = _plane(['#.#']), _plane(['#..#'])
    for radius, joins_one, joins_two in ((1, False, False), (2, True, False), (3, True, True)):
        params = link.LinkParameters(radius_xy=radius)
        assert (link.link_host(one, [1], params.reach_xy_sq, 0)[1] == 1) == joins_one
        assert (link.link_host(two, [1], params.reach_xy_sq, 0)[1] == 1) == joins_two
    for gap, mask in ((1, one), (2, two)):
        along = mask.reshape(-1, 1, 1, 1)          # the same pattern along the channel axis
        for reach_z in (0, 1, 2, 3):
            assert (link.link_host(along, _ones(along), 0, reach_z)[1] == 1) == (reach_z > gap)


def test_polarizations_are_never_joined():
    mask = np.ones((2, 2, 3, 3), np.uint8)
    labels, N0 = link.link_host(mask, [1, 1], 9, 3)
    assert N0 == 2
    assert np.all(labels[:, 0] == 1) and np.all(labels[:, 1] == 2)


def test_unfilled_channels():
    mask = np.ones((3, 1, 1, 2), np.uint8)
    filled = np.array([1, 0, 1], np.uint8)
    labels, N0 = link.link_host(mask, filled, 1, 1)
    assert N0 == 2 and np.all(labels[1] == 0) and np.all(labels[0] == 1) and np.all(labels[2] == 2)
    # the distance counts channels, filled or not
    labels, N0 = link.link_host(mask, filled, 1, 2)
    assert N0 == 1 and np.all(labels[1] == 0) and np.all(labels[0] == 1) and np.all(labels[2] == 1)


def test_u_and_spiral():
    for mask in (cases.u_shape(), cases.spiral(9), cases.spiral(16)):
        labels, N0 = link.link_host(mask, [1], 1, 0)
        assert N0 == 1
        cases.assert_same_bits(labels, mask.astype(np.int32))
        cases.assert_same_bits(labels, cases.restate(mask, [1], None, 1, 0)[0])


def test_serpentine_and_combs():
    mask = cases.serpentine(5, 7, 6)
    assert link.link_host(mask, _ones(mask), 1, 1)[1] == 1
    assert link.link_host(mask, _ones(mask), 1, 0)[1] == 5
    cases.assert_same_bits(link.link_host(mask, _ones(mask), 1, 1)[0], cases.restate(mask, _ones(mask), None, 1, 1)[0])
    mask = cases.combs(4, (2, 5, 6))
    assert link.link_host(mask, _ones(mask), 1, 1)[1] == 2
    assert link.link_host(mask[:3], np.ones(3), 1, 1)[1] == 2 * 3 * 3


def test_numbering_by_smallest_dense_index():
    mask = _plane(['..#.#', '#.#..', '#...#'])
    labels, N0 = link.link_host(mask, [1], 1, 0)
    assert N0 == 4
    assert labels[0, 0].tolist() == [[0, 0, 1, 0, 2], [3, 0, 1, 0, 0], [3, 0, 0, 0, 4]]
    table = link.measure_host(labels, np.zeros(mask.shape, np.float32), [1])
    assert table['first'].tolist() == [2, 4, 5, 14]
    assert np.all(np.diff(table['first']) > 0)


def test_peak_ties_and_signed_zero():
    labels = np.ones((1, 1, 2, 3), np.int32)
    cube = np.array([[[[1.0, 5.0, -2.0], [5.0, -2.0, 0.0]]]], np.float32)
    table = link.measure_host(labels, cube, [1])
    assert (table['peak'][0], table['peak_index'][0]) == (5.0, 1)
    assert (table['trough'][0], table['trough_index'][0]) == (-2.0, 2)
    cube = np.array([[[[0.0, -0.0, 0.0], [-0.0, 0.0, -0.0]]]], np.float32)
    table = link.measure_host(labels, cube, [1])
    assert table['peak_index'][0] == 0 and not np.signbit(table['peak'][0])
    assert table['trough_index'][0] == 1 and np.signbit(table['trough'][0])
    assert cases.key(-0.0) < cases.key(0.0)
    assert np.array_equal(link.value_keys(np.array([-1.0, -0.0, 0.0, 1.0], np.float32)),
                          [cases.key(v) for v in (-1.0, -0.0, 0.0, 1.0)])


def test_source_without_finite_values():
    labels = np.array([[[[1, 1, 0, 2]]]], np.int32)
    cube = np.array([[[[np.nan, np.inf, 7.0, 3.0]]]], np.float32)
    table = link.measure_host(labels, cube, [1])
    assert table['voxels'].tolist() == [2, 1] and table['finite'].tolist() == [0, 1]
    assert np.isnan(table['peak'][0]) and np.isnan(table['trough'][0])
    assert table['peak_index'][0] == -1 and table['trough_index'][0] == -1
    assert [table[name][0] for name in cases.SUM_FIELDS] == [0, 0, 0, 0]
    catalogue = link.catalogue_host(table, labels.shape, [1.4e9])
    assert np.all(np.isnan(catalogue['centroid'][0])) and np.isnan(catalogue['frequency'][0])
    assert catalogue['peak_c'][0] == -1 and catalogue['peak_x'][1] == 3
    assert catalogue['centroid'][1].tolist() == [0.0, 0.0, 3.0] and catalogue['frequency'][1] == 1.4e9


def test_catalogue_positions_and_frequency():
    labels = np.zeros((4, 2, 3, 5), np.int32)
    labels[1:3, 1, 2, 3] = 1
    cube = np.zeros(labels.shape, np.float32)
    cube[1, 1, 2, 3], cube[2, 1, 2, 3] = 1.0, 3.0
    table = link.measure_host(labels, cube, np.ones(4))
    catalogue = link.catalogue_host(table, labels.shape, [10.0, 20.0, 40.0, 80.0])
    row = catalogue[0]
    assert (row['id'], row['polarization'], row['voxels']) == (1, 1, 2)
    assert (row['peak_c'], row['peak_y'], row['peak_x']) == (2, 2, 3)
    assert (row['trough_c'], row['trough_y'], row['trough_x']) == (1, 2, 3)
    assert row['centroid'].tolist() == [1.75, 2.0, 3.0] and row['sum'] == 4.0
    assert row['frequency'] == 20.0 + 0.75 * 20.0


def test_filter_limits_and_renumbering():
    mask = _plane(['#..##..#', '....#..#', '.......#'])
    labels, N0 = link.link_host(mask, [1], 1, 0)
    assert N0 == 3
    table = link.measure_host(labels, np.ones(mask.shape, np.float32), [1])
    assert table['voxels'].tolist() == [1, 3, 3]
    same, same_table = link.filter_host(labels, table)
    cases.assert_same_bits(same, labels)
    cases.assert_same_bits(same_table, table)
    for minima, kept in (((1, 1, 1), [1, 2, 3]), ((2, 1, 1), [2, 3]), ((3, 1, 1), [2, 3]), ((4, 1, 1), []),
                         ((1, 2, 1), [2]), ((1, 3, 1), []), ((1, 1, 2), [])):
        got, got_table = link.filter_host(labels, table, *minima)
        assert got_table['first'].tolist() == [table['first'][k - 1] for k in kept], minima
        for new, old in enumerate(kept, 1):
            assert np.array_equal(got == new, labels == old), minima
        assert got.max() == len(kept)
    tall = np.ones((2, 1, 1, 1), np.uint8)
    labels, _ = link.link_host(tall, [1, 1], 0, 1)
    table = link.measure_host(labels, np.ones(tall.shape, np.float32), [1, 1])
    assert len(link.filter_host(labels, table, min_size_z=2)[1]) == 1
    assert len(link.filter_host(labels, table, min_size_z=3)[1]) == 0


def test_label_mask():
    labels = np.array([[[[0, 1, 2, 2, 0, 3]]]], np.int32)
    assert link.label_mask_host(labels)[0, 0, 0].tolist() == [0, 1, 1, 1, 0, 1]
    assert link.label_mask_host(labels, 2)[0, 0, 0].tolist() == [0, 0, 1, 1, 0, 0]
    assert link.label_mask_host(labels, 4).sum() == 0
    assert link.label_mask_host(labels).dtype == np.uint8


def test_parameters():
    params = link.LinkParameters()
    assert (params.radius_xy, params.radius_z, params.reach_xy_sq, params.min_voxels, params.min_size_xy,
            params.min_size_z, params.max_sources, params.filters) == (1.0, 1, 1, 1, 1, 1, 65536, False)
    for radius, reach in ((0, 0), (1, 1), (1.4, 1), (1.5, 2), (2, 4), (2.9, 8), (3, 9)):
        assert link.LinkParameters(radius_xy=radius).reach_xy_sq == reach
    assert link.LinkParameters(min_size_z=2).filters
    assert 'radius_xy=1.5' in repr(link.LinkParameters(radius_xy=1.5))
    for bad in (dict(radius_xy=-0.1), dict(radius_xy=3.1), dict(radius_xy=float('nan')), dict(radius_xy='x'),
                dict(radius_xy=True), dict(radius_xy=None), dict(radius_z=-1), dict(radius_z=4),
                dict(radius_z=1.5), dict(radius_z=True), dict(min_voxels=0), dict(min_voxels=True),
                dict(min_voxels=1.5), dict(min_size_xy=0), dict(min_size_xy=False), dict(min_size_z=0),
                dict(min_size_z='a'), dict(max_sources=0), dict(max_sources=True), dict(max_sources=2 ** 24 + 1)):
        with pytest.raises((ValueError, TypeError)):
            link.LinkParameters(**bad)


def test_twin_rejections():
    mask = np.ones((2, 1, 2, 2), np.uint8)
    labels = np.ones((2, 1, 2, 2), np.int32)
    cube = np.ones((2, 1, 2, 2), np.float32)
    with pytest.raises(TypeError):
        link.link_host(mask.astype(np.int32), [1, 1])
    for bad in (lambda: link.link_host(mask[0], [1]), lambda: link.link_host(mask, [1]),
                lambda: link.link_host(mask, [1, 1], 10, 1), lambda: link.link_host(mask, [1, 1], 1, 4),
                lambda: link.link_host(mask, [1, 1], -1, 1), lambda: link.link_host(mask, [1, 1], True, 1),
                lambda: link.measure_host(labels.astype(np.int64), cube, [1, 1]),
                lambda: link.measure_host(labels, cube.astype(np.float64), [1, 1]),
                lambda: link.measure_host(labels, cube[:1], [1, 1]),
                lambda: link.measure_host(labels, cube, [1]),
                lambda: link.filter_host(labels, np.zeros(1), 1, 1, 1),
                lambda: link.filter_host(labels, np.zeros(0, link.TABLE_DTYPE)),
                lambda: link.filter_host(labels, np.zeros(1, link.TABLE_DTYPE), min_voxels=0),
                lambda: link.filter_host(labels, np.zeros(1, link.TABLE_DTYPE), min_size_xy=True),
                lambda: link.label_mask_host(labels, -1), lambda: link.label_mask_host(labels, True),
                lambda: link.label_mask_host(labels.astype(np.uint8))):
        with pytest.raises(ValueError):
            bad()
    err = link.TooManySources(7, 5)
    assert (err.count, err.max_sources, err.labels) == (7, 5, None) and '7' in str(err)
