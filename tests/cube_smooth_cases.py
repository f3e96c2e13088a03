"""What the two cube-smoothing test modules share: the float64 direct convolution and its bound, the
cubes and tap tables of the device-against-twin cases, and the argument errors of kimg_cube_smooth."""
import ctypes

import numpy as np

from helpers import SENTINELS

EINVAL = -10001
EUNSUPPORTED = -10002
QUIET_NAN = 0x7fc00000
#: the radii the cases draw from
RADII = (0, 1, 2, 3, 7, 16)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def direct(plane, taps, R):
    """One channel [P][H][W] convolved in float64 with the float32 ``taps`` as they are:
    ``(d, S)``, ``d = sum k I`` and ``S = sum |k| |I|`` per pixel, zeros beyond the plane."""
    P, H, W = plane.shape
    D = 2 * R + 1
    padded = np.zeros((P, H + 2 * R, W + 2 * R), np.float64)
    padded[:, R:R + H, R:R + W] = plane
    d = np.zeros(plane.shape, np.float64)
    S = np.zeros(plane.shape, np.float64)
    with np.errstate(all='ignore'):
        for iy in range(D):
            for ix in range(D):
                k = np.float64(taps[iy * D + ix])
                part = padded[:, iy:iy + H, ix:ix + W]
                d += k * part
                S += abs(k) * np.abs(part)
    return d, S


def bound(R, S):
    """|t - d| <= ((2R + 1)^2 + 1) 2^-24 sum |k| |I|: (2R + 1)^2 products rounded once each and as
    many sums, each of which rounds a partial sum that is at most sum |k| |I| (1 + 2^-24)^n -- to
    first order n + 1 half-ulps of S for the n = (2R + 1)^2 terms; the +1 absorbs the second order
    (n 2^-24 <= 1089 x 6e-8)."""
    return ((2 * R + 1) ** 2 + 1) * 2.0 ** -24 * S


def assert_within_bound(got, cube, filled, radius, taps, where=None):
    """``got`` [C][P][H][W] against the float64 convolution wherever that is finite; returns the
    number of values that were (a small plane under a wide kernel can be all NaN)."""
    checked = 0
    for c in np.flatnonzero(filled):
        R = int(radius[c])
        d, S = direct(cube[c], taps[c], R)
        ok = np.isfinite(S) & np.isfinite(d)
        checked += int(ok.sum())
        if not ok.any():
            assert not np.isfinite(got[c]).any(), where
            continue
        error = np.abs(got[c].astype(np.float64)[ok] - d[ok])
        assert (error <= bound(R, S)[ok]).all(), (where, int(c), float(error.max()))
        # where an Inf or a NaN is in the footprint the result is not finite either
        assert not np.isfinite(got[c][~np.isfinite(S)]).any(), where
    return checked


def make_case(C, plane, seed, radii=None):
    """``(cube float32 [C][P][H][W], filled uint8 [C], radius int32 [C], taps float32 [C][1089])``:
    magnitudes in [1e-3, 1e3] of either sign with a few NaN and Inf, one channel not filled when
    there are two or more, radii drawn from RADII (all of them over the channels of one cube when
    there are enough), taps of either sign, and NaN in the entries of the table a channel does not use."""
    rng = np.random.default_rng(seed)
    shape = (C,) + tuple(plane)
    cube = (10.0 ** rng.uniform(-3.0, 3.0, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
    n = cube.size
    flat = cube.reshape(-1)
    odd = np.array([0x7fc12345, 0xffc00001, 0x7f800000, 0xff800000], np.uint32).view(np.float32)
    for i, value in enumerate(odd):
        if n > 4 * (i + 1):
            flat[rng.integers(0, n)] = value
    filled = np.ones(C, np.uint8)
    if C >= 2:
        filled[(seed + 1) % C] = 0
    if radii is None:
        radii = [RADII[(seed + c) % len(RADII)] for c in range(C)]
    radius = np.array(radii, np.int32)
    taps = np.full((C, 33 * 33), np.nan, np.float32)
    for c in range(C):
        count = (2 * int(radius[c]) + 1) ** 2
        taps[c, :count] = (rng.uniform(-0.3, 1.0, count) * 1.3 / count).astype(np.float32)
    return cube, filled, radius, taps


# ---- the device runs (nothing of the package is imported until one is made) --------------------------

#: (pad of the channel pitch, offset of the view into the buffer), in floats
LAYOUTS = ((0, 0), (3, 0), (4, 0), (0, 1))
OUT_PAD = 4
SENTINEL = SENTINELS[np.dtype(np.float32)]


def form(plane, pad, offset):
    """What kimg_cube_smooth picks for cubes in 16-byte aligned buffers: 'vector' (16-byte loads and
    stores) when the base, both pitches and W are multiples of 4 floats, else 'scalar'.  (OUT_PAD
    keeps the second buffer's alignment the first's.)"""
    M = int(np.prod(plane))
    return 'vector' if offset % 4 == 0 and (M + pad) % 4 == 0 and plane[2] % 4 == 0 else 'scalar'


class PaddedCube:
    """[C][P][H][W] inside a flat device buffer of sentinels: `offset` floats in, channel pitch
    P * H * W + pad.  ``inner`` None: sentinels inside as well."""

    def __init__(self, ctx, q, shape, inner, pad, offset):
        from katsdpimager_amd import accel
        C = shape[0]
        self.shape = tuple(shape)
        self.M = int(np.prod(shape[1:]))
        self.pitch = self.M + pad
        self.host = np.full(offset + C * self.pitch, SENTINEL, np.float32)
        self.inside = np.zeros(self.host.shape, bool)
        self.inside[offset:].reshape(C, self.pitch)[:, :self.M] = True
        if inner is not None:
            self.host[self.inside] = inner.reshape(-1)
        self.whole = accel.DeviceArray(ctx, self.host.shape, np.float32)
        self.whole.set(q, self.host)
        view = self.whole.tensor[offset:].view(C, self.pitch)[:, :self.M].unflatten(1, shape[1:])
        self.array = accel.DeviceArray(ctx, shape, np.float32, tensor=view)

    def get(self, q):
        """The cube; the padding must be what it was, byte for byte."""
        out = self.whole.get(q)
        assert np.array_equal(out.view(np.uint32)[~self.inside], self.host.view(np.uint32)[~self.inside]), \
            'the padding changed'
        return out[self.inside].reshape(self.shape)

    def assert_unchanged(self, q):
        assert np.array_equal(self.whole.get(q).view(np.uint32), self.host.view(np.uint32)), \
            'the cube or its padding changed'


def smooth_call(lib, q, source, target, filled, radius, taps_device, taps_pitch):
    from katsdpimager_amd._lib import check
    C, P, H, W = source.shape
    check(lib.kimg_cube_smooth(
        source.array.ptr, source.pitch, target.array.ptr, target.pitch, C, P, H, W,
        filled.ctypes.data_as(ctypes.c_void_p), radius.ctypes.data_as(ctypes.c_void_p),
        taps_device.ptr, taps_pitch, q.handle), 'kimg_cube_smooth')


def run_layouts(ctx, q, cube, filled, radius, taps, forms, where, layouts=LAYOUTS):
    """One cube on every layout against the float64 convolution and the twin; returns how many
    values were finite and checked against the bound."""
    from katsdpimager_amd import accel, smooth, _lib
    sentinels = np.full(cube.shape, SENTINEL, np.float32)
    twin = smooth.cube_smooth_host(cube, filled, radius, taps, out=sentinels)
    taps_device = accel.DeviceArray(ctx, taps.shape, np.float32)
    taps_device.set(q, taps)
    checked = 0
    for pad, offset in layouts:
        source = PaddedCube(ctx, q, cube.shape, cube, pad, offset)
        target = PaddedCube(ctx, q, cube.shape, None, pad + OUT_PAD, offset)
        forms.add(form(cube.shape[1:], pad, offset))
        smooth_call(_lib.lib(), q, source, target, filled, radius, taps_device, taps.shape[1])
        got = target.get(q)
        source.assert_unchanged(q)
        at = where + (pad, offset)
        checked += assert_within_bound(got, cube, filled, radius, taps, at)
        on = filled != 0
        assert np.array_equal(np.isnan(got[on]), np.isnan(twin[on])), at
        assert (bits(got[on])[np.isnan(got[on])] == QUIET_NAN).all(), at
        assert (got[~on] == SENTINEL).all(), at
        different = bits(got) != bits(twin)
        assert not different.any(), (at, int(different.sum()), np.argwhere(different)[:4].tolist())
    return checked


def abi_call(lib, cube, pitch, out, out_pitch, C, P, H, W, filled, radius, taps, taps_pitch, stream=None):
    return lib.kimg_cube_smooth(cube, pitch, out, out_pitch, C, P, H, W, filled, radius, taps,
                                taps_pitch, stream)


def abi_errors(lib, cube, out, taps, C=8, P=2, H=4, W=8):
    """Every argument error of kimg_cube_smooth with its code: all come before any HIP call.
    ``cube`` and ``out``: addresses of C * P * H * W floats each, 16-byte aligned, that share
    nothing, ``out`` above ``cube``; ``taps``: of C * 1089 floats.  Returns the number checked."""
    M = P * H * W
    ones = (ctypes.c_uint8 * 4097)(*([1] * 4097))
    none = (ctypes.c_uint8 * C)(*([0] * C))
    last = (ctypes.c_uint8 * C)(*([0] * (C - 1) + [1]))
    zeros = (ctypes.c_int32 * 4097)(*([0] * 4097))
    u8 = lambda table: ctypes.cast(table, ctypes.c_void_p)              # noqa: E731

    def radii(*values):
        table = (ctypes.c_int32 * C)(*(list(values) + [0] * (C - len(values))))
        keep.append(table)
        return u8(table)
    keep = []
    good = dict(cube=cube, pitch=M, out=out, out_pitch=M, C=C, P=P, H=H, W=W, filled=u8(ones),
                radius=u8(zeros), taps=taps, taps_pitch=33 * 33)
    # no filled channel: a successful call that does nothing, whatever the radii say
    assert abi_call(lib, **dict(good, filled=u8(none), radius=radii(17, -1))) == 0
    bad = [
        (dict(cube=None), EINVAL), (dict(out=None), EINVAL), (dict(filled=None), EINVAL),
        (dict(radius=None), EINVAL), (dict(taps=None), EINVAL),
        (dict(C=0), EINVAL), (dict(P=0), EINVAL), (dict(H=0), EINVAL), (dict(W=0), EINVAL),
        (dict(C=-1), EINVAL), (dict(W=-8), EINVAL),
        (dict(C=4097), EINVAL),
        (dict(radius=radii(0, -1)), EINVAL), (dict(radius=radii(0, 0, 17)), EINVAL),
        (dict(radius=radii(*([0] * (C - 1) + [17])), filled=u8(last)), EINVAL),
        (dict(pitch=M - 1), EINVAL), (dict(out_pitch=M - 1), EINVAL),
        # pitches and planes whose extent in bytes leaves int64 (a product that wraps must not pass
        # for two cubes apart)
        (dict(pitch=2 ** 61), EINVAL), (dict(out_pitch=2 ** 62 + M), EINVAL),
        (dict(pitch=(2 ** 64 + 4 * M) // (4 * (C - 1))), EINVAL),
        (dict(P=2 ** 31 - 1, H=2 ** 31 - 1, W=2 ** 31 - 1, pitch=2 ** 62, out_pitch=2 ** 62), EINVAL),
        (dict(radius=radii(1), taps_pitch=8), EINVAL), (dict(radius=radii(16), taps_pitch=1088), EINVAL),
        (dict(taps_pitch=0), EINVAL),
        (dict(cube=cube + 2), EINVAL), (dict(out=out + 2), EINVAL), (dict(taps=taps + 2), EINVAL),
        # out overlaps the cube: the cube itself, shifted by a pixel, by a channel, the same address
        # under another pitch, and from the far side
        (dict(out=cube), EINVAL), (dict(out=cube + 4, W=W - 1, pitch=M, out_pitch=M), EINVAL),
        (dict(out=cube + 4 * M), EINVAL),
        (dict(out=cube, out_pitch=M + 4, W=W - 4, pitch=M), EINVAL),
        (dict(cube=cube + 4 * M, out=cube, C=C - 1), EINVAL),
        # more polarizations than a launch has rows of workgroups
        (dict(C=1, P=65536, H=1, W=1, pitch=65536, out_pitch=65536, out=cube + (1 << 20)), EUNSUPPORTED),
    ]
    for change, code in bad:
        got = abi_call(lib, **dict(good, **change))
        assert got == code, (change, got)
    return len(bad) + 1
