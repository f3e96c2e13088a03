"""The cube operators on long bands, on the device against the numpy twins: the cases of
cube_band_cases.py (whose self-checks test_cube_band_host.py runs) through the padded buffers, layouts
and comparisons of the four sibling modules -- bits against the twin, the float64 bound of the
smoothing, sentinels around everything that is written.

What each case is there for: smoothing -- the radii beyond the first word of the kernel argument and a
grid of up to 4096 channels; statistics -- every slot count, ranges and unfilled channels on the seams
of ``filled``, 12288 groups (one workgroup a group, a second trip of the init loop) and 8192 exactly;
detection -- the boxcar's ring wrapping many times over gaps longer than the window, prune's
back-writing loops over hundreds of channels, the threshold's table read up to row 4095; linking --
chains across unfilled channels on seams, the scan with 2, 3, 4 and 8 entries a thread, the filter past
one tile of 1024 rows."""
import ctypes

import numpy as np
import pytest

import band_cases
import cube_band_cases as cases
import cube_smooth_cases
import cube_stats_cases
import detect_cases
import link_cases
from helpers import context_queue

pytestmark = pytest.mark.gpu


# ---- smoothing ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('C', cases.SMOOTH_CHANNELS)
def test_smooth_every_slot(C):
    ctx, q = context_queue()
    forms, checked = set(), 0
    for name, plane, cube, filled, radius, taps in cases.smooth_short_cases(C):
        checked += cube_smooth_cases.run_layouts(ctx, q, cube, filled, radius, taps, forms, name)
    assert forms == {'scalar', 'vector'} and checked > 200 * C


@pytest.mark.parametrize('swap', [False, True])
def test_smooth_at_the_limit(swap):
    ctx, q = context_queue()
    forms = set()
    name, plane, cube, filled, radius, taps = cases.smooth_limit_cases()[int(swap)]
    layouts = ((0, 0), (0, 1)) if plane[2] % 4 == 0 else ((3, 0),)
    checked = cube_smooth_cases.run_layouts(ctx, q, cube, filled, radius, taps, forms, name, layouts)
    assert forms == ({'scalar', 'vector'} if plane[2] % 4 == 0 else {'scalar'}) and checked > 50000


# ---- plane statistics --------------------------------------------------------------------------------

def test_stats_every_slot_count():
    from katsdpimager_amd import _lib
    ctx, q = context_queue()
    forms = set()
    for name, cube, filled, keywords, region in cases.stats_slot_cases():
        C, P = cube.shape[:2]
        G = 1 if keywords['pool_polarizations'] else P
        assert _lib.lib().kimg_cube_stats_scratch_bytes(C, G) == 4 * cases.stats_scratch_words(C * G)
        cube_stats_cases.check(ctx, q, cube, filled, keywords, region, forms, name)
    assert forms == {'scalar', 'vector'}


@pytest.mark.parametrize('C', cases.STATS_SEAM_CHANNELS)
def test_stats_on_the_seams(C):
    ctx, q = context_queue()
    forms = set()
    for name, cube, filled, keywords, region in cases.stats_seam_cases(C):
        twin = cube_stats_cases.check(ctx, q, cube, filled, keywords, region, forms, name,
                                      layouts=((0, 0), (0, 1)))
        quiet = cases.stats_quiet_groups(cube.shape, filled, keywords)
        assert not twin.count[quiet].any() and twin.count[~quiet].all(), name
    assert forms == {'scalar', 'vector'}


@pytest.mark.parametrize('which', [0, 1, 2])
def test_stats_at_the_limit(which):
    """Each launch twice through one operator: the second time over outputs full of another pattern,
    so that the groups outside the range and of unfilled channels are seen to be written -- count 0
    and the quiet NaN -- by this call."""
    from katsdpimager_amd import cube_stats, _lib
    ctx, q = context_queue()
    name, cube, filled, keywords, region = cases.stats_limit_cases()[which]
    C, P = cube.shape[:2]
    params = cube_stats.CubeStatsParameters(**keywords)
    G = params.groups(P)
    assert _lib.lib().kimg_cube_stats_scratch_bytes(C, G) == 4 * cases.stats_scratch_words(C * G)
    twin = cube_stats.cube_stats_host(cube, filled, params, region)
    op = cube_stats.CubeStatsTemplate(ctx, params).instantiate(q, cube.shape)
    source = cube_stats_cases.PaddedCube(ctx, q, cube, 0, 0)
    quiet = cases.stats_quiet_groups(cube.shape, filled, keywords)
    for turn in range(2):
        got = op(source.array, filled=filled, region=region)
        cube_stats_cases.assert_same(got, twin, name + (turn,))
        assert not got.count[quiet].any() and (got.count[~quiet] > 0).sum() >= (~quiet).sum() - G, name
        for field in cube_stats_cases.FIELDS[1:]:
            assert (cube_stats_cases.bits(getattr(got, field))[quiet] == cube_stats_cases.QUIET_NAN).all(), (name, field)
        op._out.set(q, np.full(op._out.shape, 0x3f800009, np.uint32))
        op._scratch.set(q, np.full(op._scratch.shape, 0xa5a5a5a5, np.uint32))
    source.assert_unchanged(q)


# ---- detection mask ----------------------------------------------------------------------------------

#: float and mask layouts by plane: the vector form with the mask in words, the scalar one (or the
#: vector one with a tail) with the mask in bytes
_DETECT_LAYOUTS = {(1, 3, 5): (((0, 0), (0, 0)), ((1, 0), (1, 0))), (1, 5, 12): (((0, 0), (0, 0)), ((0, 1), (1, 0))),
                   (1, 1, 61): (((3, 0), (3, 0)), ((0, 0), (0, 1))), (3, 3, 5): (((3, 0), (3, 0)), ((0, 0), (0, 0)))}


def _boxcar(ctx, q, cube, mask, filled, options, layouts, seen, where):
    from katsdpimager_amd import detect, _lib
    lib = _lib.lib()
    C, M = cube.shape[0], int(np.prod(cube.shape[1:]))
    for width, with_mask, blank in options:
        want = detect.boxcar_host(cube, filled, width, mask if with_mask else None, blank)
        for (fpad, foff), (mpad, moff) in layouts:
            seen.add((detect_cases.float_form(M, fpad, foff), detect_cases.mask_form(M, mpad, moff)))
            source = detect_cases.Padded(ctx, q, C, M, cube, fpad, foff)
            the_mask = detect_cases.Padded(ctx, q, C, M, mask, mpad, moff, np.uint8)
            target = detect_cases.Padded(ctx, q, C, M, None, fpad + 4, foff)
            _lib.check(lib.kimg_cube_boxcar(
                source.ptr, source.pitch, the_mask.ptr if with_mask else None, the_mask.pitch,
                target.ptr, target.pitch, C, M, detect_cases.host_ptr(filled), width, int(blank), q.handle),
                'boxcar')
            at = where + (width, with_mask, blank, (fpad, foff), (mpad, moff))
            target.assert_holds(q, want, filled, at)
            source.assert_unchanged(q, at)
            the_mask.assert_unchanged(q, at)


@pytest.mark.parametrize('pattern', [make.__name__ for make in band_cases.MASKS])
def test_boxcar_ring_wraps(pattern):
    ctx, q = context_queue()
    C = cases.BOXCAR_CHANNELS
    filled = getattr(band_cases, pattern)(C)
    seen = set()
    for i, plane in enumerate(cases.PLANES[:3]):
        cube, mask = cases.boxcar_case(C, plane, 20 + i)
        options = [o for k, o in enumerate(cases.boxcar_options()) if plane == (1, 5, 12) or k % 3 == i]
        _boxcar(ctx, q, cube, mask, filled, options, _DETECT_LAYOUTS[plane], seen, (pattern, plane))
    assert {f for f, _ in seen} == {'vector', 'vector+tail', 'scalar'} and {m for _, m in seen} == {'word', 'bytes'}


def test_boxcar_at_the_limit():
    ctx, q = context_queue()
    C = cases.MAX_CHANNELS
    filled = band_cases.limit_mask(C)
    seen = set()
    for i, plane in enumerate(((1, 5, 12), (1, 3, 5))):
        cube, mask = cases.boxcar_case(C, plane, 30 + i)
        _boxcar(ctx, q, cube, mask, filled, cases.boxcar_limit_options(), _DETECT_LAYOUTS[plane][:1],
                seen, ('limit', plane))
    assert seen == {('vector', 'word'), ('scalar', 'bytes')}


@pytest.mark.parametrize('C', cases.PRUNE_CHANNELS)
def test_prune_long_runs(C):
    from katsdpimager_amd import detect, _lib
    ctx, q = context_queue()
    seen = set()
    for min_channels in cases.prune_minima(C):
        mask = cases.prune_mask(C, min_channels)
        M = mask.shape[1]
        want = detect.prune_host(mask, min_channels)
        cases.check_prune(C, min_channels, mask, want)
        for pad, offset in ((0, 0), (1, 0), (0, 1)):
            seen.add(detect_cases.mask_form(M, pad, offset))
            target = detect_cases.Padded(ctx, q, C, M, mask, pad, offset, np.uint8)
            _lib.check(_lib.lib().kimg_cube_mask_prune(target.ptr, target.pitch, C, M, min_channels, q.handle),
                       'prune')
            target.assert_holds(q, want, None, (C, min_channels, pad, offset))
    assert seen == {'word', 'bytes'}


@pytest.mark.parametrize('C', [97, cases.MAX_CHANNELS])
def test_threshold_apply_reblank(C):
    from katsdpimager_amd import detect, _lib
    lib = _lib.lib()
    ctx, q = context_queue()
    s = q.handle
    filled = band_cases.straddle(C) if C == 97 else band_cases.limit_mask(C)
    P, H, W = plane = (3, 3, 5)
    M = P * H * W
    polarity = 'both' if C == 97 else 'positive'
    work, mask, sigma = cases.threshold_case(C, filled, C, polarity)
    other = detect_cases.sprinkled_cube(C, plane, C + 1)
    thresholded = detect.threshold_host(work, mask, filled, sigma, cases.THRESHOLD, polarity)
    cases.check_threshold(C, filled, work, mask, sigma, thresholded, polarity)
    reblanked = detect.reblank_host(other, work, filled)
    seen = set()
    for k, ((fpad, foff), (mpad, moff)) in enumerate((((3, 0), (3, 0)), ((0, 1), (0, 1)))):
        at = (C, (fpad, foff), (mpad, moff))
        seen.add((detect_cases.float_form(M, fpad, foff), detect_cases.mask_form(M, mpad, moff)))
        source = detect_cases.Padded(ctx, q, C, M, work, fpad, foff)
        the_mask = detect_cases.Padded(ctx, q, C, M, mask, mpad, moff, np.uint8)
        table = detect_cases.Padded(ctx, q, 1, C * 3, sigma, 0, 0)

        target = detect_cases.Padded(ctx, q, C, M, mask, mpad, moff, np.uint8)
        _lib.check(lib.kimg_cube_threshold(
            source.ptr, source.pitch, target.ptr, target.pitch, C, P, H, W, detect_cases.host_ptr(filled),
            table.ptr, 3, cases.THRESHOLD, detect.POLARITIES[polarity], s), 'threshold')
        target.assert_holds(q, thresholded, None, at + ('threshold',))

        target = detect_cases.Padded(ctx, q, C, M, other, fpad + 4, foff)
        _lib.check(lib.kimg_cube_reblank(target.ptr, target.pitch, source.ptr, source.pitch, C, M,
                                         detect_cases.host_ptr(filled), s), 'reblank')
        target.assert_holds(q, reblanked, None, at + ('reblank',))

        invert = bool(k)
        applied = detect.apply_host(work, mask, filled, invert)
        target = detect_cases.Padded(ctx, q, C, M, None, fpad + 4, foff)
        _lib.check(lib.kimg_cube_mask_apply(
            source.ptr, source.pitch, the_mask.ptr, the_mask.pitch, target.ptr, target.pitch, C, M,
            detect_cases.host_ptr(filled), int(invert), s), 'apply')
        target.assert_holds(q, applied, filled, at + ('apply', invert))
        target = detect_cases.Padded(ctx, q, C, M, work, fpad, foff)
        _lib.check(lib.kimg_cube_mask_apply(
            target.ptr, target.pitch, the_mask.ptr, the_mask.pitch, target.ptr, target.pitch, C, M,
            detect_cases.host_ptr(filled), int(invert), s), 'apply')
        target.assert_holds(q, applied, filled, at + ('apply in place', invert))

        source.assert_unchanged(q, at)
        the_mask.assert_unchanged(q, at)
        table.assert_unchanged(q, at)
    assert seen == {('vector+tail', 'word'), ('scalar', 'bytes')}


# ---- linking -----------------------------------------------------------------------------------------

@pytest.mark.parametrize('C', cases.LINK_SEAM_CHANNELS)
def test_link_across_the_seams(C):
    from katsdpimager_amd import link
    ctx, q = context_queue()
    results = {}
    for k, (name, mask, cube, filled, reach, minima) in enumerate(cases.link_seam_cases(C)):
        labels, _ = link.link_host(mask, filled, *reach)
        results[name] = cases.check_link_seam(name, labels, filled)
        link_cases.run_case(ctx, q, mask, cube, filled, reach, minima, link_cases.layouts(5)[k % 5:][:1])
    pieces = {name[2:]: r for name, r in results.items()}
    assert {p > 1 for p, _ in pieces.values()} == {True, False}


def _link_only(ctx, q, mask, filled, reach, layout, where):
    """kimg_cube_link alone against link_host: the labels in their padded buffer and the count."""
    from katsdpimager_amd import link, _lib
    C, P, H, W = mask.shape
    M = P * H * W
    want, N0 = link.link_host(mask, filled, *reach)
    cases.check_link_scan_case(where[1:], mask, filled, want, N0)
    _, (mpad, moff), (lpad, loff) = layout
    the_mask = link_cases.Padded(ctx, q, C, M, mask, mpad, moff, np.uint8)
    labels = link_cases.Padded(ctx, q, C, M, None, lpad, loff, np.int32)
    work = link_cases.scratch(ctx, C, M)
    tables = link_cases.Tables(ctx, q, 1)
    _lib.check(_lib.lib().kimg_cube_link(the_mask.ptr, the_mask.pitch, labels.ptr, labels.pitch, C, P, H, W,
                                         link_cases.host_ptr(filled), reach[0], reach[1], work.ptr,
                                         tables.counts.ptr, q.handle), 'link')
    labels.assert_holds(q, want, where)
    assert tables.counts.get(q)[0] == N0, where
    the_mask.assert_unchanged(q, where)


@pytest.mark.parametrize('C,plane', cases.LINK_SCAN_SHAPES)
def test_link_scan_past_one_round(C, plane):
    """The whole chain of entries where a source has a row (N0 in the thousands); kimg_cube_link alone
    on the cube of two workgroups a channel when every voxel of it is a source."""
    from katsdpimager_amd import link
    ctx, q = context_queue()
    assert cases.scan_entries(cases.link_blocks(C, plane))[0] >= 2
    cube = link_cases.integer_cube((C,) + tuple(plane), C)
    for k, (name, mask, filled, reach) in enumerate(cases.link_scan_cases(C, plane)):
        layout = link_cases.layouts(4)[k]
        if name[0] == 'all set' and mask.size > 100000:
            _link_only(ctx, q, mask, filled, reach, layout, ((C, plane),) + name)
            continue
        labels, N0 = link.link_host(mask, filled, *reach)
        cases.check_link_scan_case(name, mask, filled, labels, N0)
        assert link_cases.run_case(ctx, q, mask, cube, filled, reach, (1, 1, 1), [layout]) == N0


def test_filter_past_one_tile():
    from katsdpimager_amd import link
    ctx, q = context_queue()
    mask = cases.filter_runs_mask()
    filled = np.ones(mask.shape[0], np.uint8)
    cube = link_cases.integer_cube(mask.shape, 4)
    labels, N0 = link.link_host(mask, filled, 0, 1)
    assert cases.check_filter_runs(link.measure_host(labels, cube, filled)) == N0
    for k, minima in enumerate(cases.FILTER_MINIMA):
        assert link_cases.run_case(ctx, q, mask, cube, filled, (0, 1), minima, link_cases.layouts(2)[k:k + 1]) == N0
    for N0 in (1024, 1025):
        mask = cases.filter_exact_mask(N0)
        cube = link_cases.gaussian_cube(mask.shape, N0)
        for k, minima in enumerate(((1, 1, 1), (2, 1, 1))):
            assert link_cases.run_case(ctx, q, mask, cube, np.ones(41, np.uint8), (0, 0), minima,
                                       link_cases.layouts(4)[2 * k:][:2], extra_rows=0 if k else 3) == N0
