"""Moment maps on the device (csrc/moments.hip through cube.Moments) against the numpy twin
(cube.moments_host, tested on its own in test_moments_host.py), and the cube that feeds them.

The contract fixes the order of every float64 sum, the build contracts nothing into fused
multiply-adds and the float64 sqrt of the build is correctly rounded (include/kimg.h), so the device
has the twin's bits: every map is compared as uint32 patterns with NaN in the same places, moment 2
included, and count exactly.

Layouts: every C of CHANNELS x every plane of PLANES, each inside a buffer of sentinels with the
channel pitch padded by 0, 3 and 4 floats and once more starting 1 float into the buffer (_form says
which kernel form each gets: four elements per thread, that with a scalar tail, or one element per
thread).  The parameter combinations -- requested moments x select_hanning x whole band / strict
sub-range x cut (-inf, a value present in the data, a per-channel table) -- rotate over the layouts,
and every C sees all 48 of them."""
import itertools

import numpy as np
import pytest

import moments_cases as cases
from helpers import context_queue, SENTINELS

pytestmark = pytest.mark.gpu

CHANNELS = (1, 2, 3, 8, 9, 33)
PLANES = ((1, 1, 1), (1, 3, 5), (2, 7, 9), (4, 16, 16), (1, 5, 257), (3, 33, 65))
#: (pad of the channel pitch, offset of the view into the buffer), in floats
LAYOUTS = ((0, 0), (3, 0), (4, 0), (0, 1))
SUBSETS = ((0,), (0, 1, 2), (8, 9), (0, 1, 2, 8, 9))
COMBINATIONS = list(itertools.product(SUBSETS, (False, True), ('band', 'range'), ('none', 'value', 'table')))


def _form(M, pad, offset):
    """What kimg_moments picks for a float32 cube of two or more channels in a 16-byte aligned buffer
    (one channel has no pitch to speak of): 'vector' (no tail), 'vector+tail' or 'scalar'."""
    if offset % 4 or (M + pad) % 4 or M < 4:
        return 'scalar'
    return 'vector' if M % 4 == 0 else 'vector+tail'


class _PaddedCube:
    """[C][P][H][W] inside a flat device buffer of sentinels: `offset` floats in, channel pitch
    P * H * W + pad."""

    def __init__(self, ctx, q, inner, pad, offset):
        from katsdpimager_amd import accel
        C = inner.shape[0]
        self.M = int(np.prod(inner.shape[1:]))
        self.pitch = self.M + pad
        self.host = np.full(offset + C * self.pitch, SENTINELS[inner.dtype], inner.dtype)
        self.inside = np.zeros(self.host.shape, bool)
        rows = self.inside[offset:].reshape(C, self.pitch)
        rows[:, :self.M] = True
        self.host[self.inside] = inner.reshape(-1)
        self.whole = accel.DeviceArray(ctx, self.host.shape, inner.dtype)
        self.whole.set(q, self.host)
        view = self.whole.tensor[offset:].view(C, self.pitch)[:, :self.M].unflatten(1, inner.shape[1:])
        self.array = accel.DeviceArray(ctx, inner.shape, inner.dtype, tensor=view)

    def assert_unchanged(self, q):
        assert np.array_equal(self.whole.get(q).view(np.uint32), self.host.view(np.uint32)), \
            'the cube or its padding changed'


def _case(C, combination):
    """(params keywords, explicit cut kind) of one combination for a band of C channels."""
    moments, hanning, span, cut = combination
    channels = None
    if span == 'range' and C >= 2:
        channels = (1, C - 1) if C >= 3 else (0, 1)
    return dict(moments=moments, select_hanning=hanning, channels=channels), cut


@pytest.mark.parametrize('C', CHANNELS)
def test_device_against_twin(C):
    from katsdpimager_amd import cube
    ctx, q = context_queue()
    forms, seen = set(), set()
    turn = 0
    for i, plane in enumerate(PLANES):
        data, x, filled, table = cases.random_cube(C, plane, 1000 * C + i)
        finite = data[np.isfinite(data)]
        if not len(finite):
            finite = np.zeros(1, np.float32)        # (one voxel, and it holds the Inf)
        for pad, offset in LAYOUTS:
            device = _PaddedCube(ctx, q, data, pad, offset)
            forms.add(_form(device.M, pad, offset))
            for _ in range(4):
                combination = COMBINATIONS[turn % len(COMBINATIONS)]
                turn += 1
                keywords, kind = _case(C, combination)
                seen.add(combination)
                cut = {'none': None, 'value': float(finite[turn % len(finite)]), 'table': table}[kind]
                params = cube.MomentParameters(**keywords)
                op = cube.MomentsTemplate(ctx, params).instantiate(q, data.shape)
                got = op(device.array, coordinates=x, cut=cut, filled=filled, channel_width=2.5)
                host_cut = params.cut_table(C) if cut is None else \
                    (np.full(C, cut, np.float32) if kind == 'value' else cut)
                want = cube.moments_host(data, x, host_cut, filled, params, channel_width=2.5)
                where = (C, plane, pad, offset, combination)
                # maps that were not asked for are not allocated
                assert set(got) == set(params.moments) | {'count'}, where
                for key in want:
                    assert got[key].shape == plane
                    cases.assert_same_bits(got[key].get(q), want[key], where + (key,))
            device.assert_unchanged(q)
    assert forms == {'scalar', 'vector', 'vector+tail'}
    assert seen == set(COMBINATIONS)


#: a plane whose element count is a multiple of four and one whose is not, each of two workgroups in
#: its widest form: with LAYOUTS they give all three kernel forms
SEAM_PLANES = ((2, 16, 36), (1, 5, 257))


def _on_every_layout(ctx, q, data, x, cut, the_cases, check):
    """Every case (first, stop, unfilled, select_hanning) through the twin once and through the device
    on every layout of LAYOUTS: bit equality.  Returns the kernel forms that ran."""
    from katsdpimager_amd import cube
    C, plane = data.shape[0], data.shape[1:]
    devices = [(_PaddedCube(ctx, q, data, pad, offset), pad, offset) for pad, offset in LAYOUTS]
    forms = set()
    for turn, case in enumerate(the_cases):
        first, stop, unfilled, hanning = case
        filled = cases.seam_filled(C, unfilled)
        params = cube.MomentParameters(SUBSETS[-1 - turn % 2], channels=(first, stop), select_hanning=hanning)
        want = cube.moments_host(data, x, cut, filled, params, channel_width=2.5)
        check(case, want)
        op = cube.MomentsTemplate(ctx, params).instantiate(q, data.shape)
        for device, pad, offset in devices:
            got = op(device.array, coordinates=x, cut=cut, filled=filled, channel_width=2.5)
            where = (C, plane, pad, offset) + case
            assert set(got) == set(params.moments) | {'count'}, where
            for key in want:
                cases.assert_same_bits(got[key].get(q), want[key], where + (key,))
            forms.add(_form(device.M, pad, offset))
    for device, _, _ in devices:
        device.assert_unchanged(q)
    return forms


@pytest.mark.parametrize('C', cases.SEAM_CHANNELS)
def test_device_against_twin_at_the_mask_seams(C):
    """Ranges whose first channel lies on either side of the seam at 32, on it and on the seam at 64
    and whose stop is a seam, next to one, or C; the channels on the seams and the range's ends
    unfilled; NaN neighbours of the seam channels under select_hanning; peaks in the range's first and
    last channel (moments_cases.seam_cases, seam_cube)."""
    ctx, q = context_queue()
    forms, seen = set(), set()

    def check(case, want):
        cases.assert_seam_peaks(C, case, want[9], x)
        seen.add(case)
    for i, plane in enumerate(SEAM_PLANES):
        data, x, cut = cases.seam_cube(C, plane, 2000 * C + i)
        forms |= _on_every_layout(ctx, q, data, x, cut, cases.seam_cases(C), check)
    assert forms == {'scalar', 'vector', 'vector+tail'}
    # (two of a range's unfilled sets coincide where its end is the channel on the seam)
    assert seen == set(cases.seam_cases(C)) and len(seen) >= 6 * len(cases.seam_ranges(C)) - 8
    assert {case[0] for case in seen} >= {31, 32, 33} and {case[1] for case in seen} >= {63, 64, C}


def test_one_launch_at_the_longest_band():
    """4096 channels, 129 words of mask by value: the upper half of the band and all of it, the last
    channel unfilled in one and holding a peak in the other."""
    ctx, q = context_queue()
    data, x, cut = cases.limit_cube(4096)
    C = cases.LIMIT_CHANNELS
    seen = []

    def check(case, want):
        first, stop, unfilled, _ = case
        flat = want[9].reshape(-1)
        assert flat[1] == np.float32(x[C - 2])
        assert C - 1 in unfilled or flat[0] == np.float32(x[C - 1])
        seen.append(case)
    forms = _on_every_layout(ctx, q, data, x, cut, cases.limit_cases(), check)
    assert forms == {'scalar'} and len(seen) == 4


def test_spectral_cube_put_and_moments_on_another_queue():
    """The cube: NaN until filled, planes put from a device array of another queue and from the host,
    refusals before anything is copied; then the moments of the cube itself with clip_sigma, launched
    on the cube's queue and read on another one without any host wait in between."""
    from katsdpimager_amd import accel, cube
    ctx, q = context_queue()
    side = ctx.create_command_queue()
    C, plane = 9, (3, 33, 65)
    f0 = 1420405751.77
    frequencies = f0 - 2.0e4 * np.arange(C) + 5.0e4
    sc = cube.SpectralCube(ctx, q, frequencies, 3, plane[1:], channel_width=-2.0e4)
    assert sc.shape == (C,) + plane and sc.array.dtype == np.float32
    assert np.isnan(sc.get()).all() and not sc.filled.any() and np.isnan(sc.noise).all()
    data, _, _, _ = cases.random_cube(C, plane, 5)
    noise = np.linspace(0.2, 0.4, C).astype(np.float32)
    skipped = 4
    for c in range(C):
        if c == skipped:
            continue
        if c % 2:
            image = accel.DeviceArray(ctx, plane, np.float32)
            image.set(side, data[c])
            side.finish()
            sc.put(c, image, noise[c])
        else:
            sc.put(c, data[c], noise[c])
    for bad, error in (((C, data[0]), ValueError), ((-1, data[0]), ValueError), ((1.5, data[0]), ValueError),
                       (('a', data[0]), TypeError), ((0, data[0][:2]), ValueError),
                       ((0, data[0].astype(np.float64)), TypeError),
                       ((0, accel.DeviceArray(ctx, plane, np.int32)), TypeError),
                       ((skipped, data[0][:, :5]), ValueError)):
        with pytest.raises(error):
            sc.put(*bad)
    want_filled = np.ones(C, np.uint8)
    want_filled[skipped] = 0
    assert np.array_equal(sc.filled, want_filled) and np.isnan(sc.noise[skipped])
    held = sc.get()
    assert np.isnan(held[skipped]).all()
    cases.assert_same_bits(np.delete(held, skipped, 0), np.delete(data, skipped, 0))
    assert np.array_equal(sc.coordinates('frequency'), frequencies)
    velocity = sc.coordinates('velocity', f0)
    assert velocity.tolist() == [(1.0 - float(f) / f0) * 299792.458 for f in frequencies]
    with pytest.raises(ValueError):
        sc.coordinates('velocity')
    for bad in ([1.0, 1.0, 2.0], [1.0, 3.0, 2.0], [[1.0, 2.0]], [1.0, np.nan], []):
        with pytest.raises(ValueError):
            cube.SpectralCube(ctx, q, bad, 1, (4, 4))

    params = cube.MomentParameters((0, 1, 2, 8, 9), rest_frequency=f0, clip_sigma=1.5, select_hanning=True)
    op = cube.MomentsTemplate(ctx, params).instantiate(q, sc.shape)
    got = op(sc)
    # every map carries the event recorded behind the call, and get() on another queue makes that
    # queue wait for it on the device before it copies: no wait on the host in between
    waited = []
    enqueue = side.enqueue_wait_for_events
    side.enqueue_wait_for_events = lambda events: (waited.extend(events), enqueue(events))[1]
    try:
        maps = {key: got[key].get(side) for key in got}
    finally:
        del side.enqueue_wait_for_events
    ready = got['count'].ready
    assert ready is not None and all(got[key].ready is ready for key in got)
    assert waited == [ready] * len(got)
    want = cube.moments_host(data, velocity, params.cut_table(C, sc.noise, sc.filled), sc.filled, params)
    for key in want:
        cases.assert_same_bits(maps[key], want[key], key)
    assert 0 < (maps['count'] > 0).mean() < 1
    cases.assert_same_bits(sc.get(), held)
    # one channel: the width comes from the cube's channel_width, on the velocity axis
    one = cube.MomentParameters((0,), rest_frequency=f0, channels=(2, 3))
    got = cube.MomentsTemplate(ctx, one).instantiate(q, sc.shape)(sc)
    width = 2.0e4 / f0 * 299792.458
    want = cube.moments_host(data, velocity, one.cut_table(C), sc.filled, one, channel_width=width)
    cases.assert_same_bits(got[0].get(q), want[0])
    # what the operator does not take
    sc.put(0, data[0])                                          # (channel 0 loses its noise)
    with pytest.raises(ValueError):
        op(sc)
    with pytest.raises(ValueError):
        cube.MomentsTemplate(ctx, cube.MomentParameters()).instantiate(q, sc.shape)(sc)   # no rest frequency
    with pytest.raises(ValueError):
        op(sc.array)                                            # a plain array without its tables
    with pytest.raises(ValueError):
        cube.MomentsTemplate(ctx, params).instantiate(q, (C + 1,) + plane)(sc)
    with pytest.raises(TypeError):
        op(data)


def test_argument_errors_return_their_codes_without_launching():
    from katsdpimager_amd import accel, _lib
    ctx, q = context_queue()
    memory = accel.DeviceArray(ctx, (8192,), np.float32)
    memory.set(q, np.full(8192, 7.0, np.float32))
    assert memory.ptr % 16 == 0
    assert cases.abi_errors(_lib.lib(), memory.ptr) == 21
    assert (memory.get(q) == 7.0).all()


def test_driver_band_into_a_cube():
    """examples/image_channel.py --moments at a small size: the channels of a band that hold emission
    go through ``frontend.process_channel`` on the imager's queue, the model is added back to the
    residual there, and ``put(channel, imager.buffer('dirty'), result['noise'], wait_for=...)`` copies
    each into a cube on another queue; then moments 0, 1, 2 at ``clip_sigma=3``.

    Source A holds 0.5, 1, 0.5 Jy in channels 1 to 3, source B 0.3, 0.6, 0.9, 0.9, 0.6, 0.3 Jy in
    channels 5 to 10: moment 1 at A must lie on the side of moment 1 at B on which it was injected.
    Moment 0 at each source must be within noise x sqrt(n) x width of the injected integral: n the
    samples that entered at the source's pixel (the ``count`` map), width the channel width in km/s,
    and noise the quadratic mean of ``result['noise']`` over the imaged channels -- the figure a user
    has for "the noise of the images".  Why it can hold: the lines occupy disjoint channels, so in
    its own channels a source's pixel holds model + residual = its flux (the dirty peak of this
    synthetic array is right to 2e-6), while the noise estimate of those channels is the residual's
    sidelobe level; a foreign channel adds to the sum only if the other source's sidelobe at this very
    pixel stands above 3 noise estimates, and the example puts B where the PSF seen from A is
    slightly negative (-0.0008 of the peak at this size, measured), which no positive cut lets in.
    (With B at (-120, 60) px the PSF there is +0.014 against noise estimates of 0.0043 per Jy: all
    nine channels entered at both pixels and moment 0 was off by 1.05 and 0.58 Jy/beam.km/s against
    a bound of 0.18 -- one major cycle leaves the far sidelobes in the residual.)
    So the samples that enter are the source's own, 3 at A and 6 at B."""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        'examples', 'image_channel.py')
    spec = importlib.util.spec_from_file_location('image_channel_example_moments', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    results = mod.main(['--moments', '--pixels', '512', '--vis', '160000', '--minor', '300',
                        '--vis-block', '131072'])
    filled = results['filled'] != 0
    assert filled.sum() == 9 and np.all(np.isfinite(results['noise'][filled]))
    noise = float(np.sqrt(np.mean(np.square(results['noise'][filled], dtype=np.float64))))
    a, b = results['sources']['A'], results['sources']['B']
    for name, source in (('A', a), ('B', b)):
        error = abs(source['moments'][0] - source['injected'][0])
        bound = noise * np.sqrt(source['count']) * results['width']
        print('source {}: moment 0 {:.6f}, injected {:.6f}, error {:.3e}, bound {:.3e} (noise {:.3e}, n {})'.format(
            name, source['moments'][0], source['injected'][0], error, bound, noise, source['count']))
    assert all(np.isfinite(s['moments'][1]) for s in (a, b))
    assert (a['moments'][1] - b['moments'][1]) * (a['injected'][1] - b['injected'][1]) > 0
    assert a['count'] == 3 and b['count'] == 6
    for source in (a, b):
        assert abs(source['moments'][0] - source['injected'][0]) \
            <= noise * np.sqrt(source['count']) * results['width']
