"""Shared by test_moments_host.py and test_moments_gpu.py: the contract of kimg_moments
(include/kimg.h, "Moment maps") restated per voxel in Python floats -- no numpy arithmetic, no code
of katsdpimager_amd.cube -- the random cubes both suites run, and the ABI's argument errors."""
import ctypes
import math

import numpy as np

NAN32 = np.float32(np.nan)


def f32(value):
    """One rounding of a Python float to float32 (overflow to inf, as a conversion does)."""
    with np.errstate(over='ignore'):
        return np.float32(value)


def restate_voxel(spectrum, x, cut, filled, first, stop, hanning, width):
    """(moment 0, 1, 2, 8, 9, count) of one element's spectrum (a sequence of float32), every number
    a Python float (IEEE double, one rounding per operation) until the final float32."""
    def finite(c):
        return first <= c < stop and bool(filled[c]) and math.isfinite(float(spectrum[c]))
    n = 0
    S0 = S1 = S2 = 0.0
    peak = -math.inf
    peak_channel = first
    x_ref = float(x[(first + stop) // 2])
    for c in range(first, stop):
        if not finite(c):
            continue
        I = float(spectrum[c])
        s = I
        if hanning:
            a = float(spectrum[c - 1]) if finite(c - 1) else I
            b = float(spectrum[c + 1]) if finite(c + 1) else I
            s = ((0.25 * a) + (0.5 * I)) + (0.25 * b)
        if not s > float(cut[c]):
            continue
        n += 1
        d = float(x[c]) - x_ref
        S0 += I
        t = I * d
        S1 += t
        S2 += t * d
        if I > peak:
            peak, peak_channel = I, c
    if n == 0:
        return NAN32, NAN32, NAN32, NAN32, NAN32, 0
    m0 = f32(S0 * width)
    m1 = m2 = NAN32
    if S0 > 0:
        r = S1 / S0
        v = S2 / S0 - r * r
        if v < 0:
            v = 0.0
        m1 = f32(x_ref + r)
        m2 = f32(math.sqrt(v)) if v == v else NAN32
    return m0, m1, m2, f32(peak), f32(float(x[peak_channel])), n


def restate(cube, x, cut, filled, first, stop, hanning, width):
    """restate_voxel over a cube [C][...plane]: {0, 1, 2, 8, 9: float32, 'count': int32}."""
    C = cube.shape[0]
    flat = cube.reshape(C, -1)
    M = flat.shape[1]
    out = {m: np.empty(M, np.float32) for m in (0, 1, 2, 8, 9)}
    out['count'] = np.empty(M, np.int32)
    for j in range(M):
        values = restate_voxel(flat[:, j], x, cut, filled, first, stop, hanning, width)
        for key, value in zip((0, 1, 2, 8, 9, 'count'), values):
            out[key][j] = value
    return {key: value.reshape(cube.shape[1:]) for key, value in out.items()}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same_bits(got, want, where=None):
    """uint32 patterns equal, NaN in the same places (any NaN pattern is a NaN)."""
    assert got.shape == want.shape and got.dtype == want.dtype, where
    if got.dtype == np.float32:
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), where
        assert np.array_equal(bits(got)[~nan], bits(want)[~nan]), where
    else:
        assert np.array_equal(got, want), where


def random_cube(C, plane, seed):
    """A cube [C][...plane] of noise about a positive level on a 1/8 grid (so that equal values, and
    ties at the peak, are common), 20 % NaN, one Inf; x in descending km/s with uneven steps; one
    unfilled channel where there are at least 3; a per-channel cut, half of whose entries are values
    present in the data."""
    rng = np.random.default_rng(seed)
    shape = (C,) + tuple(plane)
    cube = (np.round(rng.normal(0.5, 1.0, shape) * 8) / 8).astype(np.float32)
    cube[rng.random(shape) < 0.2] = np.nan
    cube.reshape(-1)[rng.integers(cube.size)] = np.inf
    x = (1000.0 - 2.5 * np.arange(C) - rng.uniform(0.0, 1.0, C)).astype(np.float64)
    filled = np.ones(C, np.uint8)
    if C >= 3:
        filled[rng.integers(C)] = 0
    cut = rng.uniform(-1.0, 1.0, C).astype(np.float32)
    present = cube.reshape(C, -1)
    for c in range(0, C, 2):
        row = present[c][np.isfinite(present[c])]
        if len(row):
            cut[c] = row[rng.integers(len(row))]
    return cube, x, filled, cut


def abi_errors(lib, pointer):
    """Every argument error of kimg_moments with its code: all come before any HIP call, so host
    addresses (``pointer``, 16-byte aligned, any readable memory) do.  Returns the number checked."""
    EINVAL, EUNSUPPORTED = -10001, -10002
    filled = (ctypes.c_uint8 * 4096)(*([1] * 4096))
    good = dict(cube=pointer, pitch=64, C=8, M=64, first=0, stop=8, x=pointer, cut=pointer,
                filled=ctypes.cast(filled, ctypes.c_void_p), width=1.0, hanning=0, outputs=1 | 32,
                m0=pointer, m1=None, m2=None, m8=None, m9=None, count=pointer, stream=None)
    bad = [
        (dict(cube=None), EINVAL), (dict(x=None), EINVAL), (dict(cut=None), EINVAL),
        (dict(filled=None), EINVAL), (dict(C=0), EINVAL), (dict(M=-1), EINVAL),
        (dict(first=-1), EINVAL), (dict(first=8), EINVAL), (dict(first=3, stop=3), EINVAL),
        (dict(stop=9), EINVAL), (dict(pitch=63), EINVAL), (dict(width=float('nan')), EINVAL),
        (dict(outputs=0), EINVAL), (dict(outputs=64), EINVAL), (dict(outputs=2), EINVAL),
        (dict(outputs=1, m0=None), EINVAL), (dict(outputs=32, count=None), EINVAL),
        (dict(m0=pointer + 2), EINVAL),
        (dict(C=4097, stop=4097), EUNSUPPORTED), (dict(M=2 ** 31 * 256, pitch=2 ** 40), EUNSUPPORTED),
    ]
    for change, code in bad:
        a = dict(good, **change)
        got = lib.kimg_moments(a['cube'], a['pitch'], a['C'], a['M'], a['first'], a['stop'], a['x'],
                               a['cut'], a['filled'], a['width'], a['hanning'], a['outputs'], a['m0'],
                               a['m1'], a['m2'], a['m8'], a['m9'], a['count'], a['stream'])
        assert got == code, (change, got)
    # an empty plane is a successful call that does nothing
    a = dict(good, M=0)
    assert lib.kimg_moments(a['cube'], a['pitch'], a['C'], a['M'], a['first'], a['stop'], a['x'],
                            a['cut'], a['filled'], a['width'], a['hanning'], a['outputs'], a['m0'],
                            a['m1'], a['m2'], a['m8'], a['m9'], a['count'], a['stream']) == 0
    return len(bad) + 1


# ---- ranges, unfilled channels and peaks on the seams of the `filled` bit mask -----------------------
#: bands of two words exactly, of one channel and of one word and a channel more
SEAM_CHANNELS = (64, 65, 97)
#: the longest band of kimg_moments and the plane its launch runs on
LIMIT_CHANNELS = 4096
LIMIT_PLANE = (1, 3, 5)


def seam_ranges(C):
    """(first, stop): first on either side of the seam at 32, on it and on the seam at 64; stop a
    seam, a seam - 1, a seam + 1, and C."""
    stops = sorted({s + d for s in (32, 64, 96) for d in (-1, 0, 1)} | {C})
    return [(first, stop) for first in (31, 32, 33, 64) for stop in stops if first < stop <= C]


def seam_cases(C):
    """[(first, stop, unfilled channels, select_hanning)]: every range of seam_ranges with the last
    bit of words 0 and 1 (and of the range) or the first bit of words 1 and 2 (and of the range)
    unfilled, or the range's two end channels alone."""
    out = []
    for first, stop in seam_ranges(C):
        for unfilled in ((31, 63, stop - 1), (32, 64, first), (first, stop - 1)):
            for hanning in (False, True):
                out.append((first, stop, tuple(sorted({c for c in unfilled if c < C})), hanning))
    return out


def seam_filled(C, unfilled):
    filled = np.ones(C, np.uint8)
    filled[list(unfilled)] = 0
    return filled


def seam_cube(C, plane, seed):
    """(cube, x, cut): random_cube without its unfilled channel, and
      voxel 2 k      the peak of range k of seam_ranges, 64, in that range's last channel,
      voxel 2 k + 1  in its first channel,
      the last 8 voxels  a NaN in channel 31, 32, 63 or 64 between finite neighbours, and in each of
                     the two channels next to it between finite neighbours."""
    cube, x, _, cut = random_cube(C, plane, seed)
    flat = cube.reshape(C, -1)
    M = flat.shape[1]
    ranges = seam_ranges(C)
    assert M >= 2 * len(ranges) + 8 and np.shares_memory(flat, cube)
    for k, (first, stop) in enumerate(ranges):
        flat[stop - 1, 2 * k] = 64.0
        flat[first, 2 * k + 1] = 64.0
    for k, c in enumerate((31, 32, 63, 64, 30, 33, 62, 65)):
        c = min(c, C - 2)
        flat[c - 1:c + 2, M - 1 - k] = [0.75, np.nan, 1.25]
    return cube, x, cut


def assert_seam_peaks(C, case, moment9, x):
    """The twin's moment 9 says of the hand-made voxels of seam_cube what they were made for."""
    first, stop, unfilled, _ = case
    k = seam_ranges(C).index((first, stop))
    flat = moment9.reshape(-1)
    if stop - 1 not in unfilled:
        assert flat[2 * k] == np.float32(x[stop - 1])
    if first not in unfilled:
        assert flat[2 * k + 1] == np.float32(x[first])


def limit_cases():
    """[(first, stop, unfilled, select_hanning)] of the launch at LIMIT_CHANNELS: the upper half from
    one channel past the middle seam, and the whole band; channels 2047 and 2048 and one of the last
    word unfilled, and in the half band the last channel too -- the round of the channel loop that
    starts there reads the last word of the mask and the spare word behind it."""
    C = LIMIT_CHANNELS
    return [(first, stop, unfilled, hanning)
            for first, stop, unfilled in ((C // 2 + 1, C, (C // 2 - 1, C // 2, C - 9, C - 1)),
                                          (0, C, (C // 2 - 1, C // 2, C - 9)))
            for hanning in (False, True)]


def limit_cube(seed):
    """(cube, x, cut) of LIMIT_CHANNELS x LIMIT_PLANE: voxel 0 has its peak in the band's last channel,
    voxel 1 in the channel before it."""
    cube, x, _, cut = random_cube(LIMIT_CHANNELS, LIMIT_PLANE, seed)
    flat = cube.reshape(LIMIT_CHANNELS, -1)
    flat[-1, 0] = 64.0
    flat[-2, 1] = 64.0
    return cube, x, cut
