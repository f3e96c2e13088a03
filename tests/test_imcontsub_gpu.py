"""Image-plane continuum subtraction on the device (csrc/imcontsub.hip through imcontsub.ImContSub)
against the numpy twin (imcontsub.imcontsub_host, tested on its own in test_imcontsub_host.py).

Device against twin, per value: |dev - t| <= 2^-24 |t| + 1e-9 S, t the twin's value BEFORE its one
rounding to float32 and S the element's largest finite |I| -- the bound tests/test_uvcontsub_gpu.py
states and derives, at the conditioning it asks for (cond(A) <= 1e3, asserted for every cube).
Every case turned out to have the bits of the ROUNDED twin on the device -- the order of every float64
operation is the twin's, the build fuses nothing and its float64 division and sqrt are correctly
rounded (include/kimg.h) -- so bit equality is asserted on top of the bound.
Exactly equal in any case: count, the fitted set, the NaN placement, the bits of non-finite samples that are
stored unchanged, and every byte the contract says is not written -- the padding, the channels that
are not filled and, out of place, the source cube.

Layouts: those of test_moments_gpu.py -- every plane of PLANES inside a buffer of sentinels with the
channel pitch padded by 0, 3 and 4 floats and once more starting 1 float into the buffer; each runs in
place and into a second buffer whose pitch is 4 floats longer (_form says which kernel form each
gets)."""
import numpy as np
import pytest

import imcontsub_cases as cases
from helpers import context_queue, SENTINELS

pytestmark = pytest.mark.gpu

PLANES = ((1, 1, 1), (1, 3, 5), (2, 7, 9), (4, 16, 16), (1, 5, 257), (3, 33, 65))
#: (pad of the channel pitch, offset of the view into the buffer), in floats
LAYOUTS = ((0, 0), (3, 0), (4, 0), (0, 1))
#: a plane whose element count is a multiple of four and one whose is not, each of two workgroups in
#: its widest form
SEAM_PLANES = ((2, 16, 36), (1, 5, 257))
#: how much longer the channel pitch of the second buffer is
OUT_PAD = 4


def _form(M, pad, offset, outputs):
    """What kimg_imcontsub picks for float32 cubes in 16-byte aligned buffers whose maps are 16-byte
    aligned: 'vector' (no tail), 'vector+tail' or 'scalar'.  (OUT_PAD keeps the second buffer's
    alignment the first's; the coefficient maps [K][M] are dense, so their pitch is M.)"""
    if offset % 4 or (M + pad) % 4 or M < 4 or ('coefficients' in outputs and M % 4):
        return 'scalar'
    return 'vector' if M % 4 == 0 else 'vector+tail'


class _PaddedCube:
    """[C][P][H][W] inside a flat device buffer of sentinels: `offset` floats in, channel pitch
    P * H * W + pad.  ``inner`` None: sentinels inside as well."""

    def __init__(self, ctx, q, shape, inner, pad, offset):
        from katsdpimager_amd import accel
        C = shape[0]
        self.shape = tuple(shape)
        self.M = int(np.prod(shape[1:]))
        self.pitch = self.M + pad
        self.host = np.full(offset + C * self.pitch, SENTINELS[np.dtype(np.float32)], np.float32)
        self.inside = np.zeros(self.host.shape, bool)
        rows = self.inside[offset:].reshape(C, self.pitch)
        rows[:, :self.M] = True
        if inner is not None:
            self.host[self.inside] = inner.reshape(-1)
        self.whole = accel.DeviceArray(ctx, self.host.shape, np.float32)
        self.whole.set(q, self.host)
        view = self.whole.tensor[offset:].view(C, self.pitch)[:, :self.M].unflatten(1, shape[1:])
        self.array = accel.DeviceArray(ctx, shape, np.float32, tensor=view)

    def reset(self, q):
        self.whole.set(q, self.host)

    def get(self, q):
        """The cube; the padding must be what it was, byte for byte."""
        out = self.whole.get(q)
        assert np.array_equal(out.view(np.uint32)[~self.inside], self.host.view(np.uint32)[~self.inside]), \
            'the padding changed'
        return out[self.inside].reshape(self.shape)

    def assert_unchanged(self, q):
        assert np.array_equal(self.whole.get(q).view(np.uint32), self.host.view(np.uint32)), \
            'the cube or its padding changed'


def _run_layouts(ctx, q, data, filled, params, frequencies, noise, outputs, identical, forms, where):
    """One cube on every layout, in place and out of place, against the twin; ``identical`` collects
    whether each result has the bits of the rounded twin, which the callers assert."""
    from katsdpimager_amd import imcontsub
    op = imcontsub.ImContSubTemplate(ctx, params).instantiate(q, data.shape, outputs=outputs)
    sentinels = np.full(data.shape, SENTINELS[np.dtype(np.float32)], np.float32)
    reference = cases.twin(data, filled, params, frequencies, noise)
    for pad, offset in LAYOUTS:
        source = _PaddedCube(ctx, q, data.shape, data, pad, offset)
        target = _PaddedCube(ctx, q, data.shape, None, pad + OUT_PAD, offset)
        forms.add(_form(source.M, pad, offset, outputs))
        # out of place: the source is not written, nor the unfilled channels of the target
        maps = op(source.array, filled=filled, frequencies=frequencies, noise=noise, out=target.array)
        assert set(maps) == set(outputs), where
        host_maps = {key: value.get(q) for key, value in maps.items()}
        source.assert_unchanged(q)
        identical.append(cases.assert_against_twin(
            target.get(q), host_maps, data, filled, params, reference, where + (pad, offset, 'out'),
            untouched=sentinels))
        # in place: the same values
        again = op(source.array, filled=filled, frequencies=frequencies, noise=noise)
        line = source.get(q)
        identical.append(cases.assert_against_twin(
            line, {key: value.get(q) for key, value in again.items()}, data, filled, params,
            reference, where + (pad, offset, 'in')))
        assert np.array_equal(cases.bits(line)[filled != 0], cases.bits(target.get(q))[filled != 0]), where
        for key in host_maps:
            assert np.array_equal(cases.bits(again[key].get(q)), cases.bits(host_maps[key])), where


ALL_OUTPUTS = ('continuum', 'coefficients', 'rms', 'count')


@pytest.mark.parametrize('C', cases.CHANNELS)
def test_device_against_twin(C):
    from katsdpimager_amd import imcontsub
    ctx, q = context_queue()
    forms, identical = set(), []
    for order in cases.orders(C):
        for i, plane in enumerate(PLANES):
            turn = 4 * i + order
            weighting = ('none', 'noise')[turn % 2]
            axis = ('channel', 'frequency')[(turn // 2) % 2]
            data, filled, fit, frequencies, noise = cases.make_cube(C, plane, order, 1000 * C + 10 * i + order)
            params = imcontsub.ImContSubParameters(order, fit_mask=fit, axis=axis, weighting=weighting,
                                                   min_samples=None if turn % 3 else min(order + 2, C))
            assert cases.worst_cond(data, filled, params, frequencies, noise) <= 1e3
            outputs = ALL_OUTPUTS if turn % 2 else imcontsub.DEFAULT_OUTPUTS
            _run_layouts(ctx, q, data, filled, params, frequencies, noise, outputs, identical, forms,
                         (C, order, plane))
    assert forms == {'scalar', 'vector', 'vector+tail'}
    assert all(identical) and len(identical) == 48 * len(cases.orders(C))


@pytest.mark.parametrize('order', [0, 1, 2, 3])
def test_device_against_twin_at_the_workgroup_seam(order):
    """Planes of two workgroups in their widest form, 65 channels (two words of the masks and a
    channel more): the elements on either side of the seam are fitted like any other."""
    from katsdpimager_amd import imcontsub
    ctx, q = context_queue()
    forms, identical = set(), []
    C = 65
    for i, plane in enumerate(SEAM_PLANES):
        assert 256 * 4 < int(np.prod(plane)) <= 2 * 256 * 4
        data, filled, fit, frequencies, noise = cases.make_cube(C, plane, order, 5000 + 10 * i + order)
        params = imcontsub.ImContSubParameters(order, fit_mask=fit, weighting='noise')
        assert cases.worst_cond(data, filled, params, frequencies, noise) <= 1e3
        # (with coefficient maps a plane of 1285 elements has no 16-byte form: both sets of maps)
        for outputs in (ALL_OUTPUTS, imcontsub.DEFAULT_OUTPUTS):
            _run_layouts(ctx, q, data, filled, params, frequencies, noise, outputs, identical, forms,
                         (C, order, plane))
    assert forms == {'scalar', 'vector', 'vector+tail'}
    assert all(identical) and len(identical) == 32


def test_one_launch_at_the_longest_band():
    """4096 channels, two masks of 129 words by value: fit channels at both ends of the band and in the
    last word of the mask, order 3."""
    from katsdpimager_amd import imcontsub
    ctx, q = context_queue()
    data, filled, fit, frequencies, noise = cases.limit_case()
    assert data.shape[0] == imcontsub.MAX_CHANNELS == 4096
    assert fit[0] and fit[-1] and fit[-32:].sum() >= 2 and not filled[-32:].all()
    forms, identical = set(), []
    for order, axis, outputs in ((3, 'channel', ALL_OUTPUTS), (1, 'frequency', imcontsub.DEFAULT_OUTPUTS)):
        params = imcontsub.ImContSubParameters(order, fit_mask=fit, axis=axis, weighting='noise')
        assert cases.worst_cond(data, filled, params, frequencies, noise) <= 1e3
        _run_layouts(ctx, q, data, filled, params, frequencies, noise, outputs, identical, forms,
                     (4096, order))
    # (5 elements: four and a tail where the pitch is 8 floats, and no coefficient maps are asked for)
    assert forms == {'scalar', 'vector+tail'}
    assert all(identical) and len(identical) == 16


def test_python_surface():
    """A SpectralCube in place and into another one, which takes the source's filled and noise; the
    maps that were asked for and no others; weighting by the recorded noise; a fit in uneven
    frequencies; what the operator refuses."""
    from katsdpimager_amd import accel, cube, imcontsub
    ctx, q = context_queue()
    side = ctx.create_command_queue()
    C, plane, order = 9, (2, 7, 9), 1
    data, filled, fit, frequencies, noise = cases.make_cube(C, plane, order, 77)
    source = cube.SpectralCube(ctx, q, frequencies, plane[0], plane[1:])
    for c in np.flatnonzero(filled):
        source.put(int(c), data[c], noise[c])
    held = source.get()
    params = imcontsub.ImContSubParameters(order, fit_mask=fit, axis='frequency', weighting='noise')
    assert cases.worst_cond(data, filled, params, frequencies, noise) <= 1e3
    template = imcontsub.ImContSubTemplate(ctx, params)
    # out=: the source stays, the other cube takes its filled and noise
    other = cube.SpectralCube(ctx, q, frequencies, plane[0], plane[1:])
    op = template.instantiate(q, source.shape)
    maps = op(source, out=other)
    assert set(maps) == {'continuum', 'rms', 'count'}
    ready = maps['count'].ready
    assert ready is not None and all(m.ready is ready for m in maps.values())
    assert all(isinstance(m, cube.MapArray) for m in maps.values())
    host_maps = {key: value.get(side) for key, value in maps.items()}      # (another queue waits for ready)
    assert np.array_equal(cases.bits(source.get()), cases.bits(held))
    assert np.array_equal(other.filled, source.filled) and other.filled is not source.filled
    assert np.array_equal(cases.bits(other.noise), cases.bits(source.noise))
    reference = cases.twin(held, filled, params, frequencies, noise)
    cases.assert_against_twin(other.get(), host_maps, held, filled, params, reference, 'out=')
    # coefficients on request, and nothing else
    only = template.instantiate(q, source.shape, outputs=('coefficients',))(source, out=other)
    assert set(only) == {'coefficients'} and only['coefficients'].shape == (order + 1,) + plane
    cases.assert_against_twin(other.get(), {'coefficients': only['coefficients'].get(q)}, held, filled,
                              params, reference, 'coefficients')
    # in place
    again = op(source)
    cases.assert_against_twin(source.get(), {key: value.get(q) for key, value in again.items()}, held,
                              filled, params, reference, 'in place')
    assert np.array_equal(cases.bits(source.get())[filled != 0], cases.bits(other.get())[filled != 0])
    # the moments of the line cube take the cube as it is
    m0 = cube.MomentsTemplate(ctx, cube.MomentParameters((0,), axis='frequency')).instantiate(q, source.shape)(source)
    assert np.isfinite(m0[0].get(q)).any()
    # refusals
    with pytest.raises(ValueError):
        template.instantiate(q, source.shape, outputs=())
    with pytest.raises(ValueError):
        template.instantiate(q, source.shape, outputs=('continuum', 'moment0'))
    with pytest.raises(ValueError):
        template.instantiate(q, source.shape, outputs=('rms', 'rms'))
    with pytest.raises(ValueError):
        template.instantiate(q, (C + 1,) + plane)
    with pytest.raises(ValueError):
        op(source, filled=filled)
    with pytest.raises(ValueError):
        op(source.array)                                        # a plain array without its tables
    with pytest.raises(ValueError):
        op(source.array, filled=filled)                         # ... without frequencies, noise
    with pytest.raises(TypeError):
        op(source, out=other.array)
    with pytest.raises(TypeError):
        op(source.array, filled=filled, frequencies=frequencies, noise=noise, out=other)
    with pytest.raises(TypeError):
        op(data)
    with pytest.raises(ValueError):
        op(source, out=cube.SpectralCube(ctx, q, frequencies + 1.0, plane[0], plane[1:]))
    with pytest.raises(ValueError):
        op(source, out=cube.SpectralCube(ctx, q, frequencies, plane[0], (7, 10)))
    source.put(int(np.flatnonzero(fit & filled)[0]), data[0])   # (a fit channel loses its noise)
    with pytest.raises(ValueError):
        op(source)
    # a partial overlap is the library's to refuse
    buffer = accel.DeviceArray(ctx, (C + 1,) + plane, np.float32)
    buffer.zero(q)
    first = accel.DeviceArray(ctx, (C,) + plane, np.float32, tensor=buffer.tensor[:C])
    second = accel.DeviceArray(ctx, (C,) + plane, np.float32, tensor=buffer.tensor[1:])
    from katsdpimager_amd._lib import KimgError
    with pytest.raises(KimgError) as info:
        op(first, filled=filled, frequencies=frequencies, noise=noise, out=second)
    assert info.value.code == cases.EINVAL
    assert not buffer.get(q).any()


def test_argument_errors_return_their_codes_and_write_nothing():
    from katsdpimager_amd import accel, _lib
    ctx, q = context_queue()
    C, M = 8, 64
    memory = accel.DeviceArray(ctx, (2 * C * M + 8 * M,), np.float32)
    memory.set(q, np.full(memory.shape, 7.0, np.float32))
    tables = accel.DeviceArray(ctx, (5 * C,), np.float64)
    tables.set(q, np.ones(5 * C))
    assert memory.ptr % 16 == 0 and tables.ptr % 8 == 0
    checked = cases.abi_errors(_lib.lib(), memory.ptr, memory.ptr + 4 * C * M, tables.ptr,
                               memory.ptr + 8 * C * M, C, M)
    assert checked == 37
    assert (memory.get(q) == 7.0).all() and (tables.get(q) == 1.0).all()


def test_line_cube_into_moments():
    """A (1, 32, 32) cube of 24 channels: per pixel a continuum linear in the channel plus a Gaussian
    line in 6 channels, no noise.  ImContSub of order 1, then Moments((0,)) over the whole band.

    Against the twin chain (imcontsub_host, then moments_host): a sample of the device's line cube is
    within 2^-24 |t| + 1e-9 S of the unrounded twin t, and so is the rounded twin, so the two line
    cubes differ by at most e_c = 2 (2^-24 |t_c| + 1e-9 S) in channel c; moment 0 is width x the float64
    sum of the samples, rounded once, so the two moments differ by at most width x sum_c e_c plus one
    float32 rounding of each, 2^-23 |moment 0|.  (With a line cube that has the twin's bits the moments
    have them too: the moments kernel is bit-exact.)

    Without the subtraction moment 0 integrates the continuum of all 24 channels on top of the line:
    it is off the injected line integral by more than the continuum's own integral over the 6 line
    channels (the continuum is positive everywhere), and with it by less than 1e-5 of that: the cube
    has no noise, so what is left is the float32 rounding of its samples, at most 2^-24 S = 3e-7 each
    and about as much again through the fit, over 24 channels: 1.5e-5 x width against a continuum
    integral over the line channels of at least 6 x 0.3 x width."""
    from katsdpimager_amd import cube, imcontsub
    ctx, q = context_queue()
    C, plane = 24, (1, 32, 32)
    lines = (9, 15)
    rng = np.random.default_rng(24)
    frequencies = 1.42e9 + 2.0e4 * np.arange(C)
    x = np.arange(C, dtype=np.float64)
    level = rng.uniform(1.0, 3.0, plane)
    slope = rng.uniform(-0.03, 0.03, plane)
    continuum = level[None] + slope[None] * x[:, None, None, None]
    amplitude = rng.uniform(0.5, 2.0, plane)
    profile = np.zeros(C)
    profile[lines[0]:lines[1]] = np.exp(-0.5 * ((np.arange(*lines) - 11.5) / 1.2) ** 2)
    data = (continuum + amplitude[None] * profile[:, None, None, None]).astype(np.float32)
    sc = cube.SpectralCube(ctx, q, frequencies, 1, plane[1:])
    for c in range(C):
        sc.put(c, data[c], 0.01)
    width = 2.0e4
    injected = amplitude * profile.sum() * width
    moments = cube.MomentParameters((0,), axis='frequency')
    m_op = cube.MomentsTemplate(ctx, moments).instantiate(q, sc.shape)
    raw = m_op(sc)[0].get(q).astype(np.float64)
    params = imcontsub.ImContSubParameters(1, line_ranges=[lines])
    assert cases.worst_cond(data, sc.filled, params) <= 1e3
    maps = imcontsub.ImContSubTemplate(ctx, params).instantiate(q, sc.shape)(sc)
    got = m_op(sc)[0].get(q)
    t_line, _ = imcontsub.imcontsub_host_double(data, sc.filled, params)
    r_line, r_maps = imcontsub.imcontsub_host(data, sc.filled, params)
    want = cube.moments_host(r_line, frequencies, moments.cut_table(C), sc.filled, moments)[0]
    S = cases.scale(data, sc.filled)
    e = 2.0 * (2.0 ** -24 * np.abs(t_line) + 1e-9 * S[None])
    bound = width * e.sum(axis=0) + 2.0 ** -23 * np.abs(want.astype(np.float64))
    error = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert (error <= bound).all()
    # (the device's line cube has the twin's bits, and then so has moment 0)
    assert np.array_equal(cases.bits(got), cases.bits(want))
    # the continuum map is the continuum at mid-band, channel 11.5 -- to the rounding of the float32
    # samples it was fitted to (2^-24 S each; the fit of a line through 18 of them is no worse than 4 x)
    assert (np.abs(maps['continuum'].get(q) - (level + slope * 11.5)) <= 2.0 ** -22 * S).all()
    over_lines = continuum[lines[0]:lines[1]].sum(axis=0) * width
    assert (np.abs(raw - injected) > over_lines).all()
    assert (np.abs(got.astype(np.float64) - injected) < 1e-5 * over_lines).all()
