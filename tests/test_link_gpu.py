"""Source linking on the device (csrc/cube_link.hip) against the numpy twins (link.py, tested on their
own in test_link_host.py): the entries through the C ABI inside buffers of sentinels, the labels, the
counts, every integer field and the peaks by bits, the four sums equal on integer cubes and within
n * 2^-53 * sum |term| of math.fsum on Gaussian ones; then the operator end to end.

Layouts: the float pitch padded by 0, 3 and 4 floats and once more starting 1 float in; the mask pitch
padded by 0, 1, 4 and 3 bytes and once more starting 1 byte in; the label pitch padded by 0, 1 and 4
labels and once more starting 1 label in.  A workgroup of the dense launches holds 1024 elements of one
channel, so every case with C > 1 spans several, and (1, 5, 257) and (3, 33, 65) do so in one channel."""
import ctypes

import numpy as np
import pytest

import link_cases as cases
from helpers import context_queue

pytestmark = pytest.mark.gpu

CHANNELS = (1, 2, 3, 9, 33)
PLANES = ((1, 1, 1), (1, 3, 5), (2, 7, 9), (1, 5, 257), (3, 33, 65))
DENSITIES = (0.01, 0.1, 0.45)
#: (the layouts, the padded buffers, the catalogue's tables and the run of one case against the twins
#: are shared with test_cube_band_gpu.py)
_Padded = cases.Padded
_host_ptr = cases.host_ptr
_scratch = cases.scratch
_fsum_rows = cases.fsum_rows
_run_case = cases.run_case
_layouts = cases.layouts


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
