"""Spectrum statistics on the device (csrc/spectrum_stats.hip through spectrum_stats.SpectrumStats)
against the numpy twin (spectrum_stats.spectrum_stats_host, tested on its own in
test_spectrum_stats_host.py): every requested map and the line cube by bits, NaN in the same places,
whatever the layout, the load form and the kernel form.  Every cube sits inside a buffer of sentinels
that must be unchanged afterwards (or, for the target of a subtraction, changed only in the filled
channels).  Both kernel forms run on every case the resident form takes, and are compared with each
other through the twin they both have to equal.

Layouts: test_moments_gpu.py's -- the channel pitch padded by 0, 3 and 4 floats, and once more starting
1 float into the buffer: four elements per thread, that with a one-element tail, one element per thread.
A workgroup of the resident form holds 256 elements in the first form and 64 in the last; the planes
(4, 16, 16), (1, 5, 257) and (3, 33, 65) are more than one workgroup in each."""
import ctypes

import numpy as np
import pytest

import spectrum_stats_cases as cases
from helpers import context_queue, SENTINELS

pytestmark = pytest.mark.gpu

CHANNELS = (1, 2, 3, 8, 9, 33, 65, 97)
PLANES = ((1, 1, 1), (1, 3, 5), (2, 7, 9), (4, 16, 16), (1, 5, 257), (3, 33, 65))
LAYOUTS = ((0, 0), (3, 0), (4, 0), (0, 1))
SENTINEL = SENTINELS[np.dtype(np.float32)]
SUBSETS = (('median',), ('sigma',), ('min',), ('max',), ('count',), cases.FIELDS, ('median', 'sigma', 'count'))


def _form(M, pad, offset):
    if offset % 4 or (M + pad) % 4 or M < 4:
        return 'scalar'
    return 'vector' if M % 4 == 0 else 'vector+tail'


class _PaddedCube:
    """[C][P][H][W] inside a flat device buffer of sentinels: `offset` floats in, channel pitch
    P * H * W + pad.  `inner` None: sentinels throughout (a target)."""

    def __init__(self, ctx, q, shape, inner, pad, offset):
        from katsdpimager_amd import accel
        C = shape[0]
        self.shape = shape
        self.M = int(np.prod(shape[1:]))
        self.pitch = self.M + pad
        self.offset = offset
        self.host = np.full(offset + C * self.pitch, SENTINEL, np.float32)
        if inner is not None:
            self.rows(self.host)[:, :self.M] = inner.reshape(C, self.M)
        self.whole = accel.DeviceArray(ctx, self.host.shape, np.float32)
        self.whole.set(q, self.host)
        view = self.whole.tensor[offset:].view(C, self.pitch)[:, :self.M].unflatten(1, shape[1:])
        self.array = accel.DeviceArray(ctx, shape, np.float32, tensor=view)

    def rows(self, flat):
        return flat[self.offset:].reshape(self.shape[0], self.pitch)

    def assert_unchanged(self, q):
        assert np.array_equal(self.whole.get(q).view(np.uint32), self.host.view(np.uint32)), \
            'the cube or its padding changed'

    def assert_line(self, q, want, filled, where):
        """The buffer holds `want` in the filled channels and what it held before everywhere else."""
        now = self.whole.get(q)
        expect = self.host.copy()
        on = np.asarray(filled) != 0
        self.rows(expect)[on, :self.M] = want.reshape(self.shape[0], self.M)[on]
        nan = np.isnan(expect)
        assert np.array_equal(np.isnan(now), nan), where
        assert np.array_equal(now.view(np.uint32)[~nan], expect.view(np.uint32)[~nan]), where


def _forms_for(enter):
    from katsdpimager_amd import spectrum_stats
    S = int(np.sum(enter))
    return ('resident', 'streaming', 'auto') if S <= spectrum_stats.resident_limit() else ('streaming', 'auto')


def _check(ctx, q, cube, filled, keywords, where, layouts=LAYOUTS, subtract=None, forms=None, seen=None):
    """One case through the twin once and through the device in every kernel form on every layout.
    ``subtract``: None, 'in place' or 'out'.  Returns the twin's maps."""
    from katsdpimager_amd import spectrum_stats
    params = spectrum_stats.SpectrumStatsParameters(**keywords)
    twin = spectrum_stats.spectrum_stats_host(cube, filled, params, subtract=subtract is not None)
    line = None
    if subtract is not None:
        twin, line = twin
    enter = params.entering(cube.shape[0], filled)
    for form in forms or _forms_for(enter):
        op = spectrum_stats.SpectrumStatsTemplate(ctx, params, tuning={'form': form}).instantiate(q, cube.shape)
        for pad, offset in layouts:
            source = _PaddedCube(ctx, q, cube.shape, cube, pad, offset)
            at = where + (form, pad, offset)
            if subtract == 'out':
                # (a target with a pitch of its own)
                target = _PaddedCube(ctx, q, cube.shape, None, 4 - pad if pad in (0, 4) else pad, offset)
                got = op(source.array, filled=filled, subtract=True, out=target.array)
                target.assert_line(q, line, filled, at)
                source.assert_unchanged(q)
            elif subtract == 'in place':
                got = op(source.array, filled=filled, subtract=True)
                source.assert_line(q, line, filled, at)
            else:
                got = op(source.array, filled=filled)
                source.assert_unchanged(q)
            assert set(got) == set(params.outputs), at
            for name in got:
                assert got[name].shape == cube.shape[1:]
                cases.assert_same_bits(got[name].get(q), twin[name], at + (name,))
            if seen is not None:
                seen.add((form, _form(source.M, pad, offset)))
    return twin


@pytest.mark.parametrize('C', CHANNELS)
def test_device_against_twin(C):
    """Every plane on every layout in every form; the options rotate with the plane: the estimator,
    the requested maps (every single one, all of them, the default), a sub-range, exclusions that sit
    on the seams of the mask words, unfilled channels there, min_samples, subtraction."""
    ctx, q = context_queue()
    seen = set()
    for i, plane in enumerate(PLANES):
        turn = C + i
        cube = cases.noise_cube(C, plane, 1000 * C + i)
        filled = cases.seam_filled(C, turn)
        keywords = dict(estimator=cases.ESTIMATORS[turn % 2], outputs=SUBSETS[turn % len(SUBSETS)],
                        exclude_ranges=cases.seam_exclusions(C, turn), min_samples=(1, 2, 5)[turn % 3])
        if turn % 2 and C >= 3:
            keywords['channels'] = (1, C - 1)
        if C == 97 and i % 2:
            keywords['channels'] = (31, 97)         # (65 channels less the seams: the resident form too)
        subtract = (None, 'in place', 'out')[turn % 3]
        twin = _check(ctx, q, cube, filled, keywords, (C, plane), subtract=subtract, seen=seen)
        assert twin['count'].max() <= filled.sum()
    wanted = {(form, load) for form in ('streaming', 'auto') for load in ('scalar', 'vector', 'vector+tail')}
    assert seen >= wanted
    assert C == 97 or seen >= {('resident', load) for load in ('scalar', 'vector', 'vector+tail')}


@pytest.mark.parametrize('values', cases.VALUE_SETS)
def test_value_sets(values):
    """cube_stats' nine value sets laid along the channel axis, both estimators, all five maps and the
    line; every_exponent once more with all 510 values in every spectrum (streaming)."""
    ctx, q = context_queue()
    for k, (C, plane) in enumerate(((34, (2, 7, 9)), (64, (1, 8, 36)))):
        cube = cases.value_cube(values, C, plane, 11 + k)
        filled = np.ones(C, np.uint8)
        filled[5] = 0
        for estimator in cases.ESTIMATORS:
            twin = _check(ctx, q, cube, filled, dict(estimator=estimator, outputs=cases.FIELDS),
                          (values, C, estimator), layouts=((0, 0), (0, 1)), subtract=('out', 'in place')[k])
            if values == 'offset':
                assert (twin['sigma'] < 3).all() if estimator == 'mad' else (twin['sigma'] > 100).all()
            if values == 'huge' and estimator == 'mad':
                assert np.isinf(twin['sigma']).any() and not np.isnan(twin['sigma']).any()
    if values == 'every_exponent':
        cube = cases.value_cube(values, 510, (1, 2, 35), 3)
        twin = _check(ctx, q, cube, np.ones(510, np.uint8), dict(estimator='mad', outputs=cases.FIELDS),
                      (values, 510), layouts=((0, 0), (3, 0)))
        assert (twin['count'] == 510).all()


def test_neighbouring_counts_and_min_samples():
    """Lanes of one wave with n = 0, 1, 2, 3, 4, 5, S - 1 and S side by side, an all-NaN element, and
    min_samples below, among and above those n."""
    ctx, q = context_queue()
    for C, plane in ((12, (1, 8, 36)), (7, (1, 5, 13))):
        cube = cases.counts_cube(C, plane, C)
        filled = np.ones(C, np.uint8)
        for min_samples in (1, 3, C, C + 1):
            for estimator in cases.ESTIMATORS:
                twin = _check(ctx, q, cube, filled,
                              dict(estimator=estimator, min_samples=min_samples, outputs=cases.FIELDS),
                              (C, min_samples, estimator), layouts=((0, 0), (3, 0)),
                              subtract='in place' if min_samples == 3 else None)
                n = twin['count'].reshape(-1)
                assert set(n[:8].tolist()) == {0, 1, 2, 3, 4, 5, C - 1, C} and n[0] == 0
                assert np.array_equal(np.isnan(twin['median']).reshape(-1), n < min_samples)


def test_around_the_resident_limit():
    """S = L - 1, L and L + 1 entering channels (L is above 64 KiB of LDS a workgroup: the dynamic-LDS
    attribute); AUTO agrees at L + 1 and RESIDENT is refused there with KIMG_EUNSUPPORTED."""
    from katsdpimager_amd import spectrum_stats, _lib
    ctx, q = context_queue()
    L = spectrum_stats.resident_limit()
    assert L * 256 * 4 > 64 * 1024
    C = L + 3
    cube = cases.noise_cube(C, (2, 8, 18), 77)
    for S in (L - 1, L, L + 1):
        filled = np.ones(C, np.uint8)
        filled[[1, 40, 70][:C - 1 - S]] = 0
        keywords = dict(estimator='mad', channels=(1, C), outputs=cases.FIELDS)
        params = spectrum_stats.SpectrumStatsParameters(**keywords)
        assert params.entering(C, filled).sum() == S
        forms = _forms_for(params.entering(C, filled))
        assert ('resident' in forms) == (S <= L)
        _check(ctx, q, cube, filled, keywords, (S,), layouts=((0, 0), (0, 1)), forms=forms)
        if S > L:
            op = spectrum_stats.SpectrumStatsTemplate(ctx, params, tuning={'form': 'resident'}).instantiate(q, cube.shape)
            source = _PaddedCube(ctx, q, cube.shape, cube, 0, 0)
            with pytest.raises(_lib.KimgError) as error:
                op(source.array, filled=filled)
            assert str(cases.EUNSUPPORTED) in str(error.value) or error.value.args[0] == cases.EUNSUPPORTED
            source.assert_unchanged(q)


def test_the_longest_band():
    """4096 channels, 129 words of each mask by value, on a plane of (1, 3, 5): streaming."""
    ctx, q = context_queue()
    C = 4096
    cube = cases.noise_cube(C, (1, 3, 5), 4096)
    filled = np.ones(C, np.uint8)
    filled[[2047, 2048, C - 9, C - 1]] = 0
    for keywords in (dict(estimator='mad', outputs=cases.FIELDS),
                     dict(estimator='median_abs', channels=(C // 2 + 1, C), exclude_ranges=[(3000, 3100)])):
        twin = _check(ctx, q, cube, filled, keywords, (C,), layouts=((0, 0), (3, 0)),
                      forms=('streaming', 'auto'), subtract='in place')
        assert twin['count'].min() > 1500
    # few entering channels of a long band: the resident form walks the whole mask
    _check(ctx, q, cube, filled, dict(exclude_ranges=[(10, 2040), (2060, 4090)], outputs=cases.FIELDS),
           (C, 'sparse'), layouts=((0, 0),))


def test_refusals_of_the_operator():
    from katsdpimager_amd import accel, cube, spectrum_stats, _lib
    ctx, q = context_queue()
    C, plane = 6, (2, 4, 8)
    data = cases.noise_cube(C, plane, 3)
    filled = np.ones(C, np.uint8)
    params = spectrum_stats.SpectrumStatsParameters()
    op = spectrum_stats.SpectrumStatsTemplate(ctx, params).instantiate(q, data.shape)
    source = _PaddedCube(ctx, q, data.shape, data, 0, 0)
    # an out that overlaps the cube without being it: one channel further into the same buffer
    big = _PaddedCube(ctx, q, (C + 1,) + plane, None, 0, 0)
    first = accel.DeviceArray(ctx, data.shape, np.float32, tensor=big.array.tensor[:C])
    second = accel.DeviceArray(ctx, data.shape, np.float32, tensor=big.array.tensor[1:])
    with pytest.raises(_lib.KimgError):
        op(first, filled=filled, subtract=True, out=second)
    big.assert_unchanged(q)
    with pytest.raises(ValueError):
        op(source.array)
    with pytest.raises(ValueError):
        op(source.array, filled=filled, out=first)
    with pytest.raises(ValueError):
        op(source.array, filled=filled, subtract=1)
    with pytest.raises(ValueError):
        op(source.array, filled=np.ones(C + 1))
    with pytest.raises(TypeError):
        op(data, filled=filled)
    with pytest.raises(ValueError):
        op(big.array, filled=np.ones(C + 1, np.uint8))
    sc = cube.SpectralCube(ctx, q, 1.0e9 + 1.0e6 * np.arange(C), plane[0], plane[1:])
    with pytest.raises(ValueError):
        op(sc, filled=filled)
    with pytest.raises(TypeError):
        op(sc, subtract=True, out=first)
    with pytest.raises(TypeError):
        op(source.array, filled=filled, subtract=True, out=sc)
    other = cube.SpectralCube(ctx, q, 2.0e9 + 1.0e6 * np.arange(C), plane[0], plane[1:])
    with pytest.raises(ValueError):
        op(sc, subtract=True, out=other)
    for bad in (dict(form='fast'), dict(form='auto', tile=3), dict(tile=3)):
        with pytest.raises(ValueError):
            spectrum_stats.SpectrumStatsTemplate(ctx, params, tuning=bad)
    with pytest.raises(TypeError):
        spectrum_stats.SpectrumStatsTemplate(ctx, dict())
    with pytest.raises(ValueError):
        spectrum_stats.SpectrumStatsTemplate(ctx, params).instantiate(q, (C,) + plane[1:])
    with pytest.raises(ValueError):
        spectrum_stats.SpectrumStatsTemplate(
            ctx, spectrum_stats.SpectrumStatsParameters(channels=(0, C + 1))).instantiate(q, data.shape)
    source.assert_unchanged(q)


@pytest.mark.parametrize('estimator', cases.ESTIMATORS)
def test_cross_check_against_cube_stats(estimator):
    """A cube [C][70] transposed into one of 70 channels whose plane is the C samples of one pixel:
    CubeStats per plane must give this operator's count, min, max, median and sigma bit for bit."""
    from katsdpimager_amd import accel, cube_stats, spectrum_stats
    ctx, q = context_queue()
    C, plane = 48, (1, 7, 10)
    M = 70
    data = cases.noise_cube(C, plane, 31)
    data.reshape(C, M)[:, 5] = np.nan                           # an element without samples
    filled = np.ones(C, np.uint8)
    params = spectrum_stats.SpectrumStatsParameters(estimator=estimator, outputs=cases.FIELDS)
    ours = {}
    for form in ('resident', 'streaming'):
        op = spectrum_stats.SpectrumStatsTemplate(ctx, params, tuning={'form': form}).instantiate(q, data.shape)
        source = _PaddedCube(ctx, q, data.shape, data, 0, 0)
        ours[form] = {name: m.get(q).reshape(M) for name, m in op(source.array, filled=filled).items()}
    turned = np.ascontiguousarray(data.reshape(C, M).T).reshape(M, 1, 6, 8)
    other = _PaddedCube(ctx, q, turned.shape, turned, 0, 0)
    stats = cube_stats.CubeStatsTemplate(
        ctx, cube_stats.CubeStatsParameters(estimator=estimator, pool_polarizations=False)).instantiate(q, turned.shape)
    theirs = stats(other.array, filled=np.ones(M, np.uint8))
    for form, maps in ours.items():
        assert np.array_equal(maps['count'], theirs.count[:, 0].astype(np.int32))
        assert maps['count'][5] == 0 and C // 2 < maps['count'].max() <= C
        for name in ('min', 'max', 'median', 'sigma'):
            cases.assert_same_bits(maps[name], getattr(theirs, name)[:, 0], (form, name))


def test_argument_errors_return_their_codes_and_write_nothing():
    from katsdpimager_amd import accel, _lib
    ctx, q = context_queue()
    lib = _lib.lib()
    memory = accel.DeviceArray(ctx, (8192,), np.float32)
    memory.set(q, np.full(8192, 7.0, np.float32))
    assert memory.ptr % 16 == 0
    assert cases.abi_errors(lib, memory.ptr, q.handle) == 35
    assert (memory.get(q) == 7.0).all()
    # S = 0 is a successful call: n = 0 everywhere, NaN in the float maps and in the filled channels
    C, M = 8, 64
    ones = (ctypes.c_uint8 * C)(*([1] * C))
    zeros = (ctypes.c_uint8 * C)()
    maps = memory.ptr + 4 * 2 * C * M
    for form in (0, 1, 2):
        memory.set(q, np.full(8192, 7.0, np.float32))
        a = dict(cube=memory.ptr, pitch=M, C=C, M=M, first=0, stop=C, stat=ctypes.cast(zeros, ctypes.c_void_p),
                 filled=ctypes.cast(ones, ctypes.c_void_p), estimator=1, min_samples=1, outputs=31,
                 median=maps, sigma=maps + 4 * M, min=maps + 8 * M, max=maps + 12 * M, count=maps + 16 * M,
                 line=memory.ptr + 4 * C * M, line_pitch=M, form=form, stream=q.handle)
        assert cases.call(lib, a) == 0
        now = memory.get(q)
        assert (now[:C * M] == 7.0).all() and np.isnan(now[C * M:2 * C * M]).all()
        assert np.isnan(now[2 * C * M:2 * C * M + 4 * M]).all()
        assert not now[2 * C * M + 4 * M:2 * C * M + 5 * M].view(np.int32).any()
        assert (now[2 * C * M + 5 * M:] == 7.0).all()


def test_driver_median_subtraction_then_moments():
    """put several channels with a continuum source and a line, op(subtract=True) into another cube,
    then Moments: moment 0 equals moments_host fed the twin's subtracted cube, and the continuum is
    gone from it where the line is not."""
    from katsdpimager_amd import cube, spectrum_stats
    ctx, q = context_queue()
    C, P, H, W = 12, 2, 17, 20
    rng = np.random.default_rng(5)
    frequencies = 1.42e9 + 2.0e4 * np.arange(C)
    data = rng.normal(0.0, 0.01, (C, P, H, W)).astype(np.float32)
    data[:, :, 5, 6] += 2.0                                     # continuum
    data[:, :, 11, 12] += 1.0                                   # continuum under a line
    data[4:7, :, 11, 12] += np.array([0.5, 1.0, 0.5], np.float32)[:, np.newaxis]
    source = cube.SpectralCube(ctx, q, frequencies, P, (H, W))
    target = cube.SpectralCube(ctx, q, frequencies, P, (H, W))
    used = [c for c in range(C) if c != 9]
    for c in used:
        source.put(c, data[c], 0.01)
    params = spectrum_stats.SpectrumStatsParameters(outputs=cases.FIELDS)
    op = spectrum_stats.SpectrumStatsTemplate(ctx, params).instantiate(q, source.shape)
    held = source.get()
    got = op(source, subtract=True, out=target)
    twin, line = spectrum_stats.spectrum_stats_host(held, source.filled, params, subtract=True)
    for name in cases.FIELDS:
        cases.assert_same_bits(got[name].get(q), twin[name], name)
    assert np.array_equal(target.filled, source.filled) and target.filled[9] == 0
    assert np.array_equal(cases.bits(target.noise[used]), cases.bits(source.noise[used]))
    result = target.get()
    assert np.isnan(result[9]).all()                            # (never put, never written)
    cases.assert_same_bits(result[used], line[used])
    cases.assert_same_bits(source.get(), held)
    assert abs(twin['median'][0, 5, 6] - 2.0) < 0.02 and abs(twin['median'][0, 11, 12] - 1.0) < 0.02
    assert (twin['sigma'] < 0.03).all() and (twin['count'] == C - 1).all()
    parameters = cube.MomentParameters((0,), axis='frequency')
    moments = cube.MomentsTemplate(ctx, parameters).instantiate(q, target.shape)
    m0 = moments(target)[0].get(q)
    want = cube.moments_host(line, frequencies, parameters.cut_table(C), target.filled, parameters)[0]
    cases.assert_same_bits(m0, want)
    width = 2.0e4
    assert abs(m0[0, 11, 12] - 2.0 * width) < 0.1 * width and abs(m0[0, 5, 6]) < 0.1 * width
    # in place gives the same cube
    op(source, subtract=True)
    cases.assert_same_bits(source.get()[used], line[used])
