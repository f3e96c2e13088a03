"""Cube smoothing to a common beam on the device (csrc/cube_smooth.hip through smooth.CubeSmooth and
the C ABI) against the numpy twin (smooth.cube_smooth_host, tested on its own in
test_cube_smooth_host.py).

Device against the float64 direct convolution of the same float32 taps, per value:
|dev - d| <= ((2R + 1)^2 + 1) 2^-24 sum |k| |I| (cube_smooth_cases.bound, the bound of the host
test).  On top of that bit equality with the twin: the device takes the twin's products and sums in
the twin's order, and the build fuses nothing.  Exactly equal in any case: the NaN placement and
payload, the padding, the unfilled channels of ``out`` and the source cube, byte for byte.

Layouts: every plane inside a buffer of sentinels with the channel pitch padded by 0, 3 and 4 floats
and once more starting 1 float into the buffer; the second buffer's pitch is 4 floats longer.
cube_smooth_cases.form says which kernel form each gets."""
import numpy as np
import pytest

import cube_smooth_cases as cases
from helpers import context_queue

pytestmark = pytest.mark.gpu

#: the last three are there for the 16-byte form (W a multiple of 4): one with four polarizations, and
#: the last is two tiles by three
PLANES = ((1, 1, 1), (1, 3, 5), (2, 7, 9), (1, 5, 257), (3, 33, 65), (4, 8, 12), (1, 70, 132))
#: (the layouts, the padded cube and the run over the layouts are shared with test_cube_band_gpu.py)
_run_layouts = cases.run_layouts


@pytest.mark.parametrize('C', [1, 2, 5])
def test_device_against_twin(C):
    ctx, q = context_queue()
    forms, radii, checked = set(), set(), 0
    for i, plane in enumerate(PLANES):
        cube, filled, radius, taps = cases.make_case(C, plane, 100 * C + i)
        radii.update(int(r) for r in radius[filled != 0])
        checked += _run_layouts(ctx, q, cube, filled, radius, taps, forms, (C, plane))
    assert forms == {'scalar', 'vector'}
    assert radii == set(cases.RADII) or C < 5
    assert checked > 10000


def test_halos_across_tile_and_plane_corners():
    """Three tiles by three of 64 x 64 at R = 16 (and a smaller radius that is no multiple of 4 beside
    it): the halo of the middle tile comes from all eight neighbours, those of the outer tiles from
    beyond the plane's edges and corners; H and W are no multiples of the tile."""
    ctx, q = context_queue()
    forms = set()
    plane = (1, 131, 140)
    cube, filled, radius, taps = cases.make_case(2, plane, 7, radii=[16, 7])
    filled[:] = 1
    checked = _run_layouts(ctx, q, cube, filled, radius, taps, forms, plane)
    assert forms == {'scalar', 'vector'} and checked > 4 * 30000


def _frequency_beams(frequencies, major=2.4, minor=1.8, theta=0.6):
    from katsdpimager_amd.beam import Beam
    return [Beam(1.0, major * frequencies[0] / f, minor * frequencies[0] / f, theta) for f in frequencies]


def test_python_surface():
    """put(beam=), the default target, out=, the returned cube's common_beam, beams and noise, plain
    arrays, and the returned cube into Moments and ImContSub."""
    from katsdpimager_amd import accel, cube, imcontsub, smooth
    from katsdpimager_amd.beam import Beam
    ctx, q = context_queue()
    C, P, H, W = 6, 2, 21, 24
    rng = np.random.default_rng(11)
    # a 5 % band: the beam of the first channel is the largest, and the common beam
    frequencies = 1.4e9 * (1.0 + 0.05 * np.arange(C) / (C - 1))
    beams = _frequency_beams(frequencies)
    data = rng.normal(0.0, 1.0, (C, P, H, W)).astype(np.float32)
    noise = rng.uniform(0.5, 1.5, C).astype(np.float32)
    source = cube.SpectralCube(ctx, q, frequencies, P, (H, W))
    assert source.beams == [None] * C and source.common_beam is None
    for c in (0, 1, 2, 3, 5):
        source.put(c, data[c], noise[c], beam=beams[c])
    assert source.beams[3] is beams[3] and source.beams[4] is None and source.common_beam is None
    held = source.get()
    params = smooth.CommonBeamParameters()
    op = smooth.CubeSmoothTemplate(ctx, params).instantiate(q, source.shape)
    out = op(source)
    assert isinstance(out, cube.SpectralCube) and out is not source and out.shape == source.shape
    target = out.common_beam
    assert target.model.x_stddev.value == beams[0].model.x_stddev.value \
        and target.model.y_stddev.value == beams[0].model.y_stddev.value
    assert [b is target for b in out.beams] == [True, True, True, True, False, True]
    assert out.beams[4] is None and source.common_beam is None and source.beams[1] is beams[1]
    assert np.array_equal(out.filled, source.filled) and out.filled is not source.filled
    radius, taps = smooth.kernel_tables(source.beams, target, source.filled)
    factors = smooth.flux_factors(source.beams, target, source.filled)
    assert radius[0] == 0 and (radius[[1, 2, 3, 5]] > 0).all() and factors[0] == 1.0
    assert np.array_equal(op.radius, radius) and op.target is target
    # the noise: scaled where the plane was only scaled, NaN where it was smoothed or is not filled
    assert out.noise[0] == noise[0] and np.isnan(out.noise[1:]).all()
    want = smooth.cube_smooth_host(held, source.filled, radius, taps)
    got = out.get()
    assert np.array_equal(cases.bits(got), cases.bits(want))            # (NaN in channel 4 of both)
    assert cases.assert_within_bound(got, held, source.filled, radius, taps) > 4000
    assert np.array_equal(cases.bits(source.get()), cases.bits(held))
    # out=, another target, Jy/pixel: every plane is smoothed, none only scaled
    wide = Beam(1.0, 3.0, 2.5, 0.6)
    other = cube.SpectralCube(ctx, q, frequencies, P, (H, W))
    pixel = smooth.CubeSmoothTemplate(ctx, smooth.CommonBeamParameters(wide, truncate=3.0, units='pixel'))
    again = pixel.instantiate(q, source.shape)(source, out=other)
    assert again is other and other.common_beam is wide and np.isnan(other.noise).all()
    radius, taps = smooth.kernel_tables(source.beams, wide, source.filled, truncate=3.0, units='pixel')
    assert (radius[source.filled != 0] > 0).all()
    want = smooth.cube_smooth_host(held, source.filled, radius, taps)
    assert np.array_equal(cases.bits(other.get()), cases.bits(want))
    # truncate below 4 with a kernel sigma above 4 px: radius 14, and the factors come with it
    far = Beam(1.0, 5.0, 4.5, 0.6)
    short = smooth.CubeSmoothTemplate(ctx, smooth.CommonBeamParameters(far, truncate=3.0)).instantiate(q, source.shape)
    # ... into a cube that held planes of its own: it is taken over whole, and the plane it held in
    # a channel the source has not filled is NaN again
    other.put(4, data[4], noise[4], beam=beams[4])
    assert short(source, out=other) is other and other.common_beam is far and other.beams[4] is None
    radius, taps = smooth.kernel_tables(source.beams, far, source.filled, truncate=3.0)
    assert (radius[source.filled != 0] == 14).all() and np.array_equal(short.radius, radius)
    assert np.array_equal(short.factors[source.filled != 0],
                          smooth.flux_factors(source.beams, far, source.filled)[source.filled != 0])
    assert np.array_equal(other.filled, source.filled) and np.isnan(other.noise).all()
    want = smooth.cube_smooth_host(held, source.filled, radius, taps)
    assert np.array_equal(cases.bits(other.get()), cases.bits(want))    # (channel 4: NaN in both)
    # a plane that was only scaled keeps its noise, times the factor
    same = [beams[0] if f else None for f in source.filled]
    for c in np.flatnonzero(source.filled):
        source.put(int(c), data[c], noise[c], beam=beams[0])
    grown = Beam(1.0, beams[0].model.x_stddev.value * (1 + 2e-5), beams[0].model.y_stddev.value * (1 + 2e-5), 0.6)
    scaled = smooth.CubeSmoothTemplate(ctx, smooth.CommonBeamParameters(grown)).instantiate(q, source.shape)(source)
    factor = smooth.flux_factors(same, grown)[0]
    assert 1.0 < factor < 1.0001 and (scaled.noise[source.filled != 0]
                                      == (noise.astype(np.float64) * factor).astype(np.float32)[source.filled != 0]).all()
    assert np.isnan(scaled.noise[4])
    # plain arrays bring beams= and filled=
    plain = accel.DeviceArray(ctx, source.shape, np.float32)
    plain.set(q, held)
    result = op(plain, beams=beams, filled=source.filled)
    assert isinstance(result, accel.DeviceArray)
    radius, taps = smooth.kernel_tables(beams, beams[0], source.filled)
    assert np.array_equal(cases.bits(result.get(q)), cases.bits(smooth.cube_smooth_host(held, source.filled, radius, taps)))
    # the cube operators take the returned cube as it is
    moments = cube.MomentsTemplate(ctx, cube.MomentParameters((0,), axis='frequency')).instantiate(q, out.shape)
    m0 = moments(out)[0].get(q)
    expect = cube.moments_host(out.get(), frequencies, np.full(C, -np.inf, np.float32), out.filled,
                               cube.MomentParameters((0,), axis='frequency'))[0]
    assert np.array_equal(cases.bits(m0), cases.bits(expect)) and np.isfinite(m0).all()
    fit = imcontsub.ImContSubParameters(0, line_ranges=[(2, 3)])
    maps = imcontsub.ImContSubTemplate(ctx, fit).instantiate(q, out.shape)(out)
    assert np.isfinite(maps['continuum'].get(q)).all() and (maps['count'].get(q) == 4).all()
    # refusals
    with pytest.raises(ValueError):
        op(source, out=source)
    with pytest.raises(ValueError):
        op(source, beams=beams)
    with pytest.raises(ValueError):
        op(plain)
    with pytest.raises(ValueError):
        op(plain, beams=beams)
    with pytest.raises(TypeError):
        op(source, out=plain)
    with pytest.raises(TypeError):
        op(plain, beams=beams, filled=source.filled, out=other)
    with pytest.raises(TypeError):
        op(held)
    with pytest.raises(ValueError):
        op(source, out=cube.SpectralCube(ctx, q, frequencies + 1.0, P, (H, W)))
    with pytest.raises(ValueError):
        op(source, out=cube.SpectralCube(ctx, q, frequencies, P, (H, W + 1)))
    with pytest.raises(ValueError, match='polarizations'):
        op(source, out=cube.SpectralCube(ctx, q, frequencies, [1, 0], (H, W)))
    with pytest.raises(ValueError, match='channel width'):
        op(source, out=cube.SpectralCube(ctx, q, frequencies, P, (H, W), channel_width=1.0e6))
    with pytest.raises(ValueError):
        smooth.CubeSmoothTemplate(ctx, params).instantiate(q, (C, P, H))
    missing = cube.SpectralCube(ctx, q, frequencies, P, (H, W))
    missing.put(0, data[0], beam=beams[0])
    missing.put(1, data[1])                                     # a plane without a beam
    with pytest.raises(ValueError, match='channel 1'):
        op(missing)
    with pytest.raises(ValueError, match='does not contain'):
        smooth.CubeSmoothTemplate(ctx, smooth.CommonBeamParameters(beams[5])).instantiate(q, source.shape)(out)
    # a partial overlap is the library's to refuse
    from katsdpimager_amd._lib import KimgError
    buffer = accel.DeviceArray(ctx, (C + 1, P, H, W), np.float32)
    buffer.zero(q)
    first = accel.DeviceArray(ctx, source.shape, np.float32, tensor=buffer.tensor[:C])
    second = accel.DeviceArray(ctx, source.shape, np.float32, tensor=buffer.tensor[1:])
    with pytest.raises(KimgError) as info:
        op(first, beams=beams, filled=source.filled, out=second)
    assert info.value.code == cases.EINVAL
    assert not buffer.get(q).any()


def test_argument_errors_return_their_codes_and_write_nothing():
    from katsdpimager_amd import accel, _lib
    ctx, q = context_queue()
    C, M = 8, 64
    memory = accel.DeviceArray(ctx, (2 * C * M,), np.float32)
    memory.set(q, np.full(memory.shape, 7.0, np.float32))
    taps = accel.DeviceArray(ctx, (C * 33 * 33,), np.float32)
    taps.set(q, np.ones(taps.shape, np.float32))
    assert memory.ptr % 16 == 0 and taps.ptr % 16 == 0
    assert cases.abi_errors(_lib.lib(), memory.ptr, memory.ptr + 4 * C * M, taps.ptr) == 34
    assert (memory.get(q) == 7.0).all() and (taps.get(q) == 1.0).all()
