"""The detection mask on the device (csrc/cube_detect.hip) against the numpy twins (detect.py, tested on
their own in test_detect_host.py): the five entries through the C ABI on every layout, by bits with NaN
in the same places, and the whole finder (detect.SmoothClip) against smooth_clip_host by bytes.

Every cube and mask sits in a buffer of sentinels that must be unchanged outside what the contract
writes.  Layouts: the float pitch padded by 0, 3 and 4 floats and once more starting 1 float into the
buffer (four elements per thread, that with a one-element tail, one element per thread); the mask
pitch padded by 0, 1 and 4 bytes and once more starting 1 byte in (one 4-byte access, four byte
accesses), and by 3 bytes too: a plane whose floats have the form with a tail has M = 1 mod 4, and only
that padding gives its mask the 4-byte form; every float layout meets every mask layout.  The boxcar's
workgroup holds 256 elements in the first float form and 64 in the last; the planes (4, 16, 16),
(1, 5, 257) and (3, 33, 65) are more than one workgroup in each."""
import ctypes

import numpy as np
import pytest

import detect_cases as cases
from helpers import context_queue

pytestmark = pytest.mark.gpu

CHANNELS = (1, 2, 3, 8, 9, 33, 65)
PLANES = ((1, 1, 1), (1, 3, 5), (2, 7, 9), (4, 16, 16), (1, 5, 257), (3, 33, 65))
#: (the layouts and the padded buffers are shared with test_cube_band_gpu.py)
FLOAT_LAYOUTS = cases.FLOAT_LAYOUTS
MASK_LAYOUTS = cases.MASK_LAYOUTS
_float_form = cases.float_form
_mask_form = cases.mask_form
_Padded = cases.Padded
_host_ptr = cases.host_ptr


@pytest.mark.parametrize('C', CHANNELS)
def test_entries_against_twins(C):
    """Every plane in every float layout with every mask layout; the options rotate with the plane and
    the layout: the width (1, 3, 7, 15, 31, so also above C), with and without a mask, blank, groups,
    polarity, min_channels (1, 2, 3, C), in place or out, invert."""
    from katsdpimager_amd import detect, _lib
    lib = _lib.lib()
    ctx, q = context_queue()
    s = q.handle
    seen = set()
    for i, plane in enumerate(PLANES):
        P, H, W = plane
        M = P * H * W
        turn = C + i
        cube = cases.sprinkled_cube(C, plane, 100 * C + i)
        work = cases.sprinkled_cube(C, plane, 100 * C + i + 50)
        filled = cases.filled_for(C, turn)
        mask = cases.random_mask(cube.shape, turn, 0.3, values=(1, 1, 2, 255))
        runs = cases.run_mask(C, M, turn).reshape(cube.shape)
        twins = {}
        for k, (fpad, foff) in enumerate(FLOAT_LAYOUTS):
            for n, (mpad, moff) in enumerate(MASK_LAYOUTS):
                step = turn + 5 * k + n
                at = (C, plane, (fpad, foff), (mpad, moff))
                seen.add((_float_form(M, fpad, foff), _mask_form(M, mpad, moff)))
                other = FLOAT_LAYOUTS[(k + 1) % 4][0]       # (a target's pitch is its own)
                source = _Padded(ctx, q, C, M, cube, fpad, foff)
                the_mask = _Padded(ctx, q, C, M, mask, mpad, moff, np.uint8)

                # boxcar
                width = cases.WIDTHS[step % 5]
                with_mask, blank = bool(step & 1), bool(step & 2)
                key = ('boxcar', width, with_mask, blank)
                if key not in twins:
                    twins[key] = detect.boxcar_host(cube, filled, width, mask if with_mask else None, blank)
                target = _Padded(ctx, q, C, M, None, other, foff)
                _lib.check(lib.kimg_cube_boxcar(
                    source.ptr, source.pitch, the_mask.ptr if with_mask else None, the_mask.pitch,
                    target.ptr, target.pitch, C, M, _host_ptr(filled), width, int(blank), s), 'boxcar')
                target.assert_holds(q, twins[key], filled, at + key)

                # reblank
                if 'reblank' not in twins:
                    twins['reblank'] = detect.reblank_host(work, cube, filled)
                target = _Padded(ctx, q, C, M, work, other, foff)
                _lib.check(lib.kimg_cube_reblank(target.ptr, target.pitch, source.ptr, source.pitch, C, M,
                                                 _host_ptr(filled), s), 'reblank')
                target.assert_holds(q, twins['reblank'], None, at + ('reblank',))

                # threshold: groups 1 and P, every polarity, a table with NaN, 0 and a negative entry
                G = (1, P)[step % 2]
                polarity = cases.POLARITIES[step % 3]
                key = ('threshold', G, polarity)
                sigma = cases.sigma_table(C, G, 7)
                if key not in twins:
                    twins[key] = detect.threshold_host(cube, mask, filled, sigma, 1.25, polarity)
                table = _Padded(ctx, q, 1, C * G, sigma, 0, 0)
                target = _Padded(ctx, q, C, M, mask, mpad, moff, np.uint8)
                _lib.check(lib.kimg_cube_threshold(
                    source.ptr, source.pitch, target.ptr, target.pitch, C, P, H, W, _host_ptr(filled),
                    table.ptr, G, 1.25, detect.POLARITIES[polarity], s), 'threshold')
                target.assert_holds(q, twins[key], None, at + key)

                # prune
                min_channels = min((1, 2, 3, C)[step % 4], C)
                key = ('prune', min_channels)
                if key not in twins:
                    twins[key] = detect.prune_host(runs, min_channels)
                target = _Padded(ctx, q, C, M, runs, mpad, moff, np.uint8)
                _lib.check(lib.kimg_cube_mask_prune(target.ptr, target.pitch, C, M, min_channels, s), 'prune')
                target.assert_holds(q, twins[key], None, at + key)

                # apply
                invert, in_place = bool(step & 1), bool(step & 4)
                key = ('apply', invert)
                if key not in twins:
                    twins[key] = detect.apply_host(cube, mask, filled, invert)
                if in_place:
                    target = _Padded(ctx, q, C, M, cube, fpad, foff)
                    _lib.check(lib.kimg_cube_mask_apply(
                        target.ptr, target.pitch, the_mask.ptr, the_mask.pitch, target.ptr, target.pitch,
                        C, M, _host_ptr(filled), int(invert), s), 'apply')
                else:
                    target = _Padded(ctx, q, C, M, None, other, foff)
                    _lib.check(lib.kimg_cube_mask_apply(
                        source.ptr, source.pitch, the_mask.ptr, the_mask.pitch, target.ptr, target.pitch,
                        C, M, _host_ptr(filled), int(invert), s), 'apply')
                target.assert_holds(q, twins[key], filled, at + key + (in_place,))

                source.assert_unchanged(q, at)
                the_mask.assert_unchanged(q, at)
                table.assert_unchanged(q, at)
    assert seen == {(f, m) for f in ('vector', 'vector+tail', 'scalar') for m in ('word', 'bytes')}


@pytest.mark.parametrize('width', cases.WIDTHS)
def test_boxcar_every_option(width):
    """Every width with and without a mask and with blank 0 and 1, on a band shorter than the widest
    windows and on one longer than them, in the vector form with a tail and in the scalar one."""
    from katsdpimager_amd import detect, _lib
    lib = _lib.lib()
    ctx, q = context_queue()
    for C, plane in ((9, (2, 7, 9)), (65, (1, 5, 53))):
        M = int(np.prod(plane))
        cube = cases.sprinkled_cube(C, plane, width + C)
        filled = cases.filled_for(C, width)
        mask = cases.random_mask(cube.shape, width, 0.4, values=(1, 3))
        for with_mask in (False, True):
            for blank in (False, True):
                want = detect.boxcar_host(cube, filled, width, mask if with_mask else None, blank)
                for (fpad, foff), (mpad, moff) in (((2, 0), (2, 0)), ((0, 1), (1, 0))):
                    source = _Padded(ctx, q, C, M, cube, fpad, foff)
                    the_mask = _Padded(ctx, q, C, M, mask, mpad, moff, np.uint8)
                    target = _Padded(ctx, q, C, M, None, fpad, foff)
                    _lib.check(lib.kimg_cube_boxcar(
                        source.ptr, source.pitch, the_mask.ptr if with_mask else None, the_mask.pitch,
                        target.ptr, target.pitch, C, M, _host_ptr(filled), width, int(blank), q.handle),
                        'boxcar')
                    target.assert_holds(q, want, filled, (width, C, with_mask, blank, fpad, foff))


def test_boxcar_order_of_the_sum():
    """The cancellation triples of test_detect_host.py: the device sums ascending, in float64."""
    from katsdpimager_amd import detect, _lib
    ctx, q = context_queue()
    big = np.float32(2.0 ** 60)
    column = np.array([1.0, big, -big, 1.0, big, -big, 1.0], np.float32)
    cube = np.repeat(column.reshape(-1, 1), 8, axis=1).reshape(7, 1, 2, 4).copy()
    filled = np.ones(7, np.uint8)
    for width in (3, 5, 7):
        want = detect.boxcar_host(cube, filled, width)
        source = _Padded(ctx, q, 7, 8, cube, 0, 0)
        target = _Padded(ctx, q, 7, 8, None, 0, 0)
        _lib.check(_lib.lib().kimg_cube_boxcar(source.ptr, 8, None, 0, target.ptr, 8, 7, 8,
                                               _host_ptr(filled), width, 0, q.handle), 'boxcar')
        target.assert_holds(q, want, None, width)
    assert detect.boxcar_host(cube, filled, 3)[1, 0, 0, 0] == 0 and detect.boxcar_host(cube, filled, 3)[2, 0, 0, 0] != 0


def test_abi_rejections():
    from katsdpimager_amd import _lib
    ctx, q = context_queue()
    P = ctypes.c_void_p
    cube = _Padded(ctx, q, 4, 16, cases.sprinkled_cube(4, (1, 4, 4), 1), 0, 0)
    out = _Padded(ctx, q, 4, 16, cases.sprinkled_cube(4, (1, 4, 4), 2), 0, 0)
    mask = _Padded(ctx, q, 4, 16, cases.random_mask((4, 16), 3), 0, 0, np.uint8)
    sigma = _Padded(ctx, q, 1, 4, np.ones(4, np.float32), 0, 0)
    filled = np.ones(4097, np.uint8)
    calls = cases.abi_rejections(_lib.lib(), P(cube.ptr), P(mask.ptr), P(out.ptr), P(sigma.ptr),
                                 _host_ptr(filled), q.handle)
    q.finish()
    wrong = [(name, got, want) for name, got, want in calls if got != want]
    assert not wrong, wrong
    assert {want for _, _, want in calls} == {0, cases.EINVAL, cases.EUNSUPPORTED}
    cube.assert_unchanged(q, 'cube')
    sigma.assert_unchanged(q, 'sigma')


# ---- the whole finder --------------------------------------------------------------------------------

def _finder_cases():
    for estimator in cases.ESTIMATORS:
        for pool in (True, False):
            yield estimator, pool


@pytest.mark.parametrize('estimator,pool', list(_finder_cases()))
def test_finder_against_twin(estimator, pool):
    """(16, 2, 40, 48), three unfilled channels, a NaN corner: the mask by bytes, with and without a
    region, replace on and off, min_channels 1 and 2; a second run of the same operator gives the same
    bytes (the scratch and the work cubes carry nothing over); the cube is never written."""
    from katsdpimager_amd import accel, detect
    ctx, q = context_queue()
    cube, filled, region = cases.finder_cube()
    array = accel.DeviceArray(ctx, cube.shape, np.float32)
    array.set(q, cube)
    other = np.where(np.isfinite(cube), -cube, cube).astype(np.float32)
    for replace in (True, False):
        for min_channels in (1, 2):
            params = detect.SmoothClipParameters(
                spatial_fwhm=(0, 3), spectral_widths=(1, 3, 7), threshold=3.5, estimator=estimator,
                pool_polarizations=pool, replace=replace, min_channels=min_channels, border=2)
            op = detect.SmoothClipTemplate(ctx, params).instantiate(q, cube.shape)
            for use in (None, region):
                at = (estimator, pool, replace, min_channels, use is not None)
                want = detect.smooth_clip_host(cube, filled, params, use)
                assert want.any() and want.mean() < 0.1
                mask = op(array, filled=filled, region=use)
                assert isinstance(mask, detect.MaskCube) and mask.shape == cube.shape
                cases.assert_same_bits(mask.get(q), want, at)
                again = op(array, filled=filled, region=use)
                cases.assert_same_bits(again.get(q), want, at + ('again',))
            # ... also after another cube went through the operator
            array2 = accel.DeviceArray(ctx, cube.shape, np.float32)
            array2.set(q, other)
            op(array2, filled=np.ones(len(filled), np.uint8))
            cases.assert_same_bits(op(array, filled=filled).get(q),
                                   detect.smooth_clip_host(cube, filled, params), 'after another cube')
    cases.assert_same_bits(array.get(q), cube, 'the cube')


def test_finder_polarities_and_pitch():
    """'negative' and 'both' on a cube that is a view with a channel pitch of its own."""
    from katsdpimager_amd import accel, detect
    ctx, q = context_queue()
    cube, filled, region = cases.finder_cube()
    C = cube.shape[0]
    M = int(np.prod(cube.shape[1:]))
    padded = _Padded(ctx, q, C, M, cube, 4, 0)
    view = padded.whole.tensor.view(C, M + 4)[:, :M].unflatten(1, cube.shape[1:])
    array = accel.DeviceArray(ctx, cube.shape, np.float32, tensor=view)
    for polarity in ('negative', 'both'):
        params = detect.SmoothClipParameters(spatial_fwhm=(3, 0), spectral_widths=(3, 1), threshold=3.0,
                                             polarity=polarity)
        want = detect.smooth_clip_host(cube, filled, params)
        got = detect.SmoothClipTemplate(ctx, params).instantiate(q, cube.shape)(array, filled=filled)
        cases.assert_same_bits(got.get(q), want, polarity)
        assert want.any()
    padded.assert_unchanged(q, 'the cube')


def test_faint_source_and_moments():
    """The point of the feature: a source whose peak lies below threshold x sigma in every voxel is
    not seen by the per-voxel clip and is found -- and nothing away from it -- by the full kernel set;
    then the mask applied to the cube and moment 0 of that, against the twins by bits."""
    from katsdpimager_amd import cube as cube_module, detect
    ctx, q = context_queue()
    data, filled = cases.faint_cube()
    C, P, H, W = data.shape
    frequencies = 1.4e9 + 1e5 * np.arange(C)
    the_cube = cube_module.SpectralCube(ctx, q, frequencies, P, (H, W))
    for c in range(C):
        the_cube.put(c, data[c], noise=1.0)
    single_params = detect.SmoothClipParameters(spatial_fwhm=(0,), spectral_widths=(1,),
                                                threshold=cases.FAINT_THRESHOLD)
    full_params = detect.SmoothClipParameters(threshold=cases.FAINT_THRESHOLD)
    single = detect.SmoothClipTemplate(ctx, single_params).instantiate(q, data.shape)(the_cube)
    full = detect.SmoothClipTemplate(ctx, full_params).instantiate(q, data.shape)(the_cube)
    single_host, full_host = single.get(q), full.get(q)
    cases.assert_faint_source(single_host, full_host)
    cases.assert_same_bits(single_host, detect.smooth_clip_host(data, filled, single_params))
    cases.assert_same_bits(full_host, detect.smooth_clip_host(data, filled, full_params))

    params = cube_module.MomentParameters(moments=(0,), axis='frequency')
    moments = cube_module.MomentsTemplate(ctx, params).instantiate(q, data.shape)
    for invert in (False, True):
        masked = full.apply(the_cube, invert=invert)
        assert masked is not the_cube and np.array_equal(masked.filled, the_cube.filled)
        assert np.array_equal(masked.noise, the_cube.noise)
        want_cube = detect.apply_host(data, full_host, filled, invert)
        cases.assert_same_bits(masked.get(), want_cube, ('apply', invert))
        want = cube_module.moments_host(want_cube, frequencies, params.cut_table(C), filled, params)
        got = moments(masked)
        cases.assert_same_bits(got[0].get(q), want[0], ('moment 0', invert))
        cases.assert_same_bits(got['count'].get(q), want['count'], ('count', invert))
    # the source's flux is in the map through the mask, and nowhere else
    through = cube_module.moments_host(detect.apply_host(data, full_host, filled), frequencies,
                                       params.cut_table(C), filled, params)
    assert through['count'][0, cases.FAINT_CENTRE[1], cases.FAINT_CENTRE[2]] >= 3
    assert (through['count'] > 0).sum() == full_host.any(axis=0).sum()
    # in place
    cases.assert_same_bits(the_cube.get(), data, 'the cube before')
    assert full.apply(the_cube, out=the_cube) is the_cube
    cases.assert_same_bits(the_cube.get(), detect.apply_host(data, full_host, filled), 'in place')
