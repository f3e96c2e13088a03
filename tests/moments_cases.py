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

