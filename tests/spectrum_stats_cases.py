"""Shared by test_spectrum_stats_host.py and test_spectrum_stats_gpu.py: the contract of
kimg_spectrum_stats (include/kimg.h, "Spectrum statistics") restated per voxel in plain Python -- a
sorted list of (key, value), the two middle elements, np.float32 arithmetic, no code of the package --,
the cubes both suites run, and the ABI's argument errors."""
import ctypes
import struct

import numpy as np

import cube_stats_cases

EINVAL = -10001
EUNSUPPORTED = -10002
FIELDS = ('median', 'sigma', 'min', 'max', 'count')
OUTPUT_BITS = {'median': 1, 'sigma': 2, 'min': 4, 'max': 8, 'count': 16}
ESTIMATORS = ('median_abs', 'mad')
NAN32 = np.float32(np.nan)
TO_RMS = np.float32(1.4826022185056031)
#: elements a workgroup of the resident form holds, in its 16-byte form
RESIDENT_TILE = 256


def _bits(value):
    return struct.unpack('<I', struct.pack('<f', float(value)))[0]


def _key(value):
    b = _bits(value)
    return b ^ (0xffffffff if b >> 31 else 0x80000000)


def _median(values, key):
    """(v[(n - 1) // 2] + v[n // 2]) / 2 in float32 of float32 values ordered by `key`."""
    ordered = sorted(((key(v), v) for v in values), key=lambda pair: pair[0])
    n = len(ordered)
    lo, hi = ordered[(n - 1) // 2][1], ordered[n // 2][1]
    with np.errstate(all='ignore'):
        return np.float32(np.float32(lo + hi) / np.float32(2)), ordered


def restate_voxel(spectrum, enter, estimator, min_samples):
    """(median, sigma, min, max, count) of one element's spectrum (a sequence of float32); ``enter``
    [C] says which channels enter."""
    samples = [np.float32(x) for x, e in zip(spectrum, enter) if e and np.isfinite(x)]
    n = len(samples)
    if n < min_samples or n == 0:
        return NAN32, NAN32, NAN32, NAN32, n
    m, ordered = _median(samples, _key)
    with np.errstate(all='ignore'):
        if estimator == 'mad':
            spread = [np.abs(np.float32(x - m)) for x in samples]
        else:
            spread = [np.abs(x) for x in samples]
        s, _ = _median(spread, lambda v: 0x80000000 | _bits(v))
        sigma = np.float32(s * TO_RMS)
    return m, sigma, ordered[0][1], ordered[-1][1], n


def restate(cube, enter, filled, estimator, min_samples, subtract=False):
    """restate_voxel over a cube [C][...plane]: {field: [...plane]} and, with ``subtract``, the line
    cube: every filled channel minus the median, NaN where the median is."""
    C = cube.shape[0]
    flat = cube.reshape(C, -1)
    M = flat.shape[1]
    out = {name: np.empty(M, np.int32 if name == 'count' else np.float32) for name in FIELDS}
    for j in range(M):
        for name, value in zip(FIELDS, restate_voxel(flat[:, j], enter, estimator, min_samples)):
            out[name][j] = value
    maps = {name: value.reshape(cube.shape[1:]) for name, value in out.items()}
    if not subtract:
        return maps
    line = flat.copy()
    for c in range(C):
        if filled[c]:
            for j in range(M):
                m = out['median'][j]
                with np.errstate(all='ignore'):
                    line[c, j] = NAN32 if np.isnan(m) else np.float32(flat[c, j] - m)
    return maps, line.reshape(cube.shape)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same_bits(got, want, where=None):
    """uint32 patterns equal, NaN in the same places (any NaN pattern is a NaN)."""
    assert got.shape == want.shape and got.dtype == want.dtype, where
    if got.dtype == np.float32:
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), where
        different = (bits(got) != bits(want)) & ~nan
        assert not different.any(), (where, np.argwhere(different)[:4].tolist(),
                                     got[different][:4].tolist(), want[different][:4].tolist())
    else:
        assert np.array_equal(got, want), where


# ---- cubes -------------------------------------------------------------------------------------------
VALUE_SETS = tuple(sorted(cube_stats_cases.VALUE_SETS))


def value_cube(values, C, plane, seed):
    """One of cube_stats' value sets laid along the channel axis: cube_stats makes it for M groups of
    C samples (what varies from channel to channel there varies from pixel to pixel here), and the
    transpose is the cube [C][...plane]."""
    M = int(np.prod(plane))
    rng = np.random.default_rng(seed)
    groups = cube_stats_cases.VALUE_SETS[values](rng, (M, 1, 1, C))
    return np.ascontiguousarray(groups.reshape(M, C).T).reshape((C,) + tuple(plane))


def noise_cube(C, plane, seed, nan_fraction=0.15):
    """Noise on a 1/8 grid about a level that differs per pixel (ties are common), some NaN, one +Inf
    and one -Inf."""
    rng = np.random.default_rng(seed)
    shape = (C,) + tuple(plane)
    level = rng.normal(0.0, 4.0, (1,) + tuple(plane))
    cube = (np.round((level + rng.normal(0.0, 1.0, shape)) * 8) / 8).astype(np.float32)
    cube[rng.random(shape) < nan_fraction] = np.nan
    flat = cube.reshape(-1)
    flat[rng.integers(flat.size)] = np.inf
    flat[rng.integers(flat.size)] = -np.inf
    return cube


def counts_cube(C, plane, seed):
    """Noise whose NaN pattern gives neighbouring elements n = 0, 1, 2, 3, 4, 5, C - 1 and C finite
    samples, side by side and repeating along the plane; which channels are finite differs from
    element to element.  Element 0 is all NaN."""
    rng = np.random.default_rng(seed)
    M = int(np.prod(plane))
    cube = rng.normal(0.0, 1.0, (C, M)).astype(np.float32)
    wanted = (0, 1, 2, 3, 4, 5, C - 1, C)
    for j in range(M):
        n = min(max(wanted[j % len(wanted)], 0), C)
        gone = rng.permutation(C)[:C - n]
        cube[gone, j] = np.nan
    return cube.reshape((C,) + tuple(plane))


def seam_filled(C, turn):
    """Every channel but those on the seams of the mask words: the last bit of words 0 and 1 or the
    first of words 1 and 2, by turns; none unfilled in a band of one channel."""
    filled = np.ones(C, np.uint8)
    for c in ((31, 63), (32, 64), (0, C - 1))[turn % 3]:
        if c < C and C > 1:
            filled[c] = 0
    return filled


def seam_exclusions(C, turn):
    """None, or ranges that end and start on the seams (the non-entering channels sit there)."""
    if C < 9:
        return (None, [(0, 1)], [(C - 1, C)])[turn % 3] if C >= 3 else None
    choices = (None, [(30, 33)], [(63, 65), (2, 4)], [(31, 32), (64, 65)])
    ranges = choices[turn % len(choices)]
    if ranges is None:
        return None
    kept = [(a, min(b, C)) for a, b in ranges if a < C]
    return kept or None


# ---- the ABI's argument errors ---------------------------------------------------------------------
def call(lib, a):
    return lib.kimg_spectrum_stats(
        a['cube'], a['pitch'], a['C'], a['M'], a['first'], a['stop'], a['stat'], a['filled'],
        a['estimator'], a['min_samples'], a['outputs'], a['median'], a['sigma'], a['min'], a['max'],
        a['count'], a['line'], a['line_pitch'], a['form'], a['stream'])


def abi_errors(lib, pointer, stream=None, elements=8192):
    """Every argument error of kimg_spectrum_stats with its code: all come before any HIP call.
    ``pointer``: 16-byte aligned memory of ``elements`` floats (the maps and the cube are laid out in
    it; nothing may be written).  Returns the number checked."""
    ones = (ctypes.c_uint8 * 4097)(*([1] * 4097))
    table = ctypes.cast(ones, ctypes.c_void_p)
    C, M = 8, 64
    assert elements >= 3 * C * M
    maps = pointer + 4 * 2 * C * M
    good = dict(cube=pointer, pitch=M, C=C, M=M, first=0, stop=C, stat=table, filled=table,
                estimator=1, min_samples=1, outputs=31, median=maps, sigma=maps + 4 * M,
                min=maps + 8 * M, max=maps + 12 * M, count=maps + 16 * M, line=None, line_pitch=0,
                form=0, stream=stream)
    limit = lib.kimg_spectrum_stats_resident_limit()
    other = pointer + 4 * C * M
    bad = [
        (dict(cube=None), EINVAL), (dict(stat=None), EINVAL), (dict(filled=None), EINVAL),
        (dict(C=0), EINVAL), (dict(M=-1), EINVAL), (dict(first=-1), EINVAL), (dict(first=8), EINVAL),
        (dict(first=3, stop=3), EINVAL), (dict(stop=9), EINVAL), (dict(pitch=63), EINVAL),
        (dict(estimator=2), EINVAL), (dict(estimator=-1), EINVAL), (dict(min_samples=0), EINVAL),
        (dict(outputs=0), EINVAL), (dict(outputs=32), EINVAL), (dict(form=3), EINVAL), (dict(form=-1), EINVAL),
        (dict(cube=pointer + 2), EINVAL),
        (dict(outputs=1, median=None), EINVAL), (dict(outputs=2, sigma=None), EINVAL),
        (dict(outputs=4, min=None), EINVAL), (dict(outputs=8, max=None), EINVAL),
        (dict(outputs=16, count=None), EINVAL), (dict(sigma=maps + 4 * M + 2), EINVAL),
        # the line: needs the median map, a pitch, alignment, and no partial overlap
        (dict(line=other, line_pitch=M, outputs=30), EINVAL),
        (dict(line=other, line_pitch=M - 1), EINVAL), (dict(line=other + 2, line_pitch=M), EINVAL),
        (dict(line=pointer + 4, line_pitch=M), EINVAL), (dict(line=pointer, line_pitch=M + 4, pitch=M), EINVAL),
        (dict(line=other - 4, line_pitch=M), EINVAL),
        (dict(C=4097, stop=4097), EUNSUPPORTED), (dict(M=2 ** 31 * 64, pitch=2 ** 40), EUNSUPPORTED),
        (dict(C=limit + 1, stop=limit + 1, form=1), EUNSUPPORTED),
    ]
    for change, code in bad:
        got = call(lib, dict(good, **change))
        assert got == code, (change, got)
    # an empty plane is a successful call that does nothing
    assert call(lib, dict(good, M=0)) == 0
    assert call(lib, dict(good, M=0, line=pointer, line_pitch=M)) == 0
    return len(bad) + 2
