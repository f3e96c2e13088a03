"""What the two cube-statistics test modules share: the value sets, regions, planes and cases of the
twin-against-independent and device-against-twin tests, and the independent statement itself.

Launch geometry (csrc/cube_stats.hip): a workgroup of a pass takes 1024 loads a round -- of 4 elements
in the 16-byte form, of 1 otherwise -- and a group gets one workgroup per 1024 loads (up to a cap of
8192 workgroups a launch); a workgroup adds its histogram into slot ``workgroup % slots`` of its
group, ``slots = clamp(256 // (C * G), 1, 16)``.  MULTI_BLOCK_PLANE has 25344 elements pooled: 7
workgroups a group in the 16-byte form and 25 otherwise, so more than one workgroup per pass and more
than one slot for every C of the tests (C = 70 pooled: 3 slots)."""
import numpy as np

from helpers import SENTINELS

EINVAL = -10001
EUNSUPPORTED = -10002
QUIET_NAN = 0x7fc00000

#: the last three are there for the 16-byte form (W a multiple of 4)
PLANES = ((1, 1, 1), (1, 3, 5), (2, 7, 9), (1, 5, 257), (3, 33, 65), (4, 8, 12), (1, 70, 132))
MULTI_BLOCK_PLANE = (2, 96, 132)
#: a border of 2 leaves one pixel of each plane
ONE_PIXEL_PLANE = (2, 5, 5)
ESTIMATORS = ('median_abs', 'mad')
REGIONS = ('none', 'full', 'sparse', 'empty')
FIELDS = ('count', 'min', 'max', 'median', 'sigma')

_ODD = np.array([0x7fc12345, 0xffc00001, 0x7f800001, 0xffffffff, 0x7f800000, 0xff800000], np.uint32)
#: sets of three values whose keys part at the top byte, the second, the third and the last
_TRIPLES = np.array([[0x3f7fffff, 0x3f800000, 0x40000000],
                     [0x3f80ffff, 0x3f810000, 0x3f800000],
                     [0xbf8000ff, 0xbf800100, 0x3f8000ff],
                     [0x3f800000, 0x3f800001, 0xbf800001]], np.uint32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _floats(words):
    return np.ascontiguousarray(words, np.uint32).view(np.float32)


# ---- value sets: (rng, shape (C, P, H, W)) -> float32 cube ---------------------------------------
def noise_like(rng, shape):
    """Gaussian noise, another sigma every channel: three or four exponent bytes."""
    sigma = 10.0 ** rng.uniform(-4.0, 1.0, (shape[0], 1, 1, 1))
    return (rng.normal(0.0, 1.0, shape) * sigma).astype(np.float32)


def every_exponent(rng, shape):
    """One value from each of the 255 finite exponent bytes, both signs (510 values; a smaller
    group draws from them), random mantissas."""
    exponent = np.repeat(np.arange(255, dtype=np.uint32), 2)
    sign = np.tile(np.array([0, 1], np.uint32), 255)
    n = int(np.prod(shape))
    pick = np.concatenate([rng.permutation(510) for _ in range(n // 510 + 1)])[:n]
    mantissa = rng.integers(0, 1 << 23, n, dtype=np.uint32)
    return _floats((sign[pick] << 31) | (exponent[pick] << 23) | mantissa).reshape(shape)


def repeated(rng, shape):
    """One value, another every channel."""
    value = rng.normal(0.0, 3.0, (shape[0], 1, 1, 1)).astype(np.float32)
    return np.broadcast_to(value, shape).copy()


def three_values(rng, shape):
    """Values from a set of three, another set every channel: ties straddle every byte boundary."""
    cube = np.empty(shape, np.float32)
    for c in range(shape[0]):
        cube[c] = _floats(_TRIPLES[c % len(_TRIPLES)])[rng.integers(0, 3, shape[1:])]
    return cube


def denormals(rng, shape):
    sign = rng.integers(0, 2, shape, dtype=np.uint32) << 31
    return _floats(sign | rng.integers(0, 1 << 23, shape, dtype=np.uint32)).reshape(shape)


def zeros_mixed(rng, shape):
    """+0 and -0, and in every second channel a few other values around them."""
    cube = _floats(rng.integers(0, 2, shape, dtype=np.uint32) << 31).reshape(shape).copy()
    for c in range(1, shape[0], 2):
        other = rng.random(shape[1:]) < 0.3
        cube[c][other] = rng.normal(0.0, 1.0, int(other.sum())).astype(np.float32)
    return cube


def non_finite(rng, shape):
    """Noise with NaN of both signs and odd payloads, +Inf and -Inf sprinkled in (a third of it);
    the last channel is all NaN."""
    cube = noise_like(rng, shape)
    odd = rng.random(shape) < 0.33
    cube[odd] = _floats(_ODD)[rng.integers(0, len(_ODD), int(odd.sum()))]
    cube[-1] = _floats(_ODD[:4])[rng.integers(0, 4, shape[1:])]
    return cube


def offset(rng, shape):
    """An offset a hundred times the scatter ('mad' against 'median_abs'), either sign."""
    level = rng.choice([-100.0, 100.0], (shape[0], 1, 1, 1))
    return (level + rng.normal(0.0, 1.0, shape)).astype(np.float32)


def huge(rng, shape):
    """Values whose differences and sums overflow: x - m and lo + hi may be infinite."""
    return (rng.choice([-3.0e38, 3.0e38, 3.3e38, -3.3e38, 1.0], shape)).astype(np.float32)


VALUE_SETS = {f.__name__: f for f in (noise_like, every_exponent, repeated, three_values, denormals,
                                      zeros_mixed, non_finite, offset, huge)}


def make_region(kind, rng, H, W):
    """None, or uint8 [H][W]: all ones, about a quarter (values other than 1 among them), none; an
    integer: that many pixels."""
    if kind == 'none':
        return None
    if kind == 'full':
        return np.ones((H, W), np.uint8)
    if kind == 'empty':
        return np.zeros((H, W), np.uint8)
    if kind == 'sparse':
        return ((rng.random((H, W)) < 0.25) * rng.integers(1, 256, (H, W))).astype(np.uint8)
    region = np.zeros(H * W, np.uint8)
    region[rng.choice(H * W, int(kind), replace=False)] = 255
    return region.reshape(H, W)


def make_filled(C, seed):
    """Every channel but one (of two or more), and but every fifth of ten or more."""
    filled = np.ones(C, np.uint8)
    if C >= 2:
        filled[(seed + 1) % C] = 0
    if C >= 10:
        filled[seed % 5::5] = 0
    return filled


def make_case(C, plane, seed, values='noise_like', region='none', sprinkle=True):
    """``(cube float32 [C][P][H][W], filled uint8 [C], region)``.  ``sprinkle``: a few non-finite
    values on top of the value set, where the cube has room."""
    rng = np.random.default_rng(seed)
    shape = (C,) + tuple(plane)
    cube = VALUE_SETS[values](rng, shape)
    if sprinkle:
        flat = cube.reshape(-1)
        for i, value in enumerate(_floats(_ODD)):
            if flat.size > 4 * (i + 1):
                flat[rng.integers(0, flat.size)] = value
    return cube, make_filled(C, seed), make_region(region, rng, plane[1], plane[2])


def modes():
    """Every (pool_polarizations, estimator, border, region kind): 2 x 2 x 2 x 4."""
    return [(pool, estimator, border, region) for pool in (True, False) for estimator in ESTIMATORS
            for border in (0, 1) for region in REGIONS]


def border_fits(border, plane):
    return 2 * border < min(plane[1], plane[2])


def host_cases():
    """``(name, cube, filled, parameter keywords, region)`` of the twin's test: every plane under a
    rotating mode, every mode on two planes, every value set under both estimators and groupings,
    the ranges, the tiny groups."""
    seed = 0
    all_modes = modes()
    for i, plane in enumerate(PLANES + (ONE_PIXEL_PLANE,)):
        for C in (1, 5):
            pool, estimator, border, region = all_modes[(7 * i + C) % len(all_modes)]
            if not border_fits(border, plane):
                border = 0
            seed += 1
            cube, filled, mask = make_case(C, plane, seed, region=region)
            yield ('plane', plane, C), cube, filled, dict(
                estimator=estimator, border=border, pool_polarizations=pool), mask
    for plane in ((2, 7, 9), (4, 8, 12)):
        for pool, estimator, border, region in all_modes:
            seed += 1
            cube, filled, mask = make_case(3, plane, seed, 'non_finite', region, sprinkle=False)
            yield ('mode', plane, pool, estimator, border, region), cube, filled, dict(
                estimator=estimator, border=border, pool_polarizations=pool), mask
    for values in VALUE_SETS:
        for plane in ((2, 7, 9), (1, 5, 257)):
            for estimator in ESTIMATORS:
                for pool in (True, False):
                    seed += 1
                    cube, filled, mask = make_case(4, plane, seed, values, sprinkle=values == 'noise_like')
                    yield ('values', values, plane, estimator, pool), cube, filled, dict(
                        estimator=estimator, pool_polarizations=pool), mask
    for channels in ((0, 1), (2, 5), (6, 7), (1, 7)):
        seed += 1
        cube, filled, mask = make_case(7, (2, 7, 9), seed)
        yield ('range', channels), cube, filled, dict(channels=channels, estimator='mad'), mask
    for estimator in ESTIMATORS:
        for k in (1, 2, 3):
            seed += 1
            cube, filled, mask = make_case(3, (1, 7, 9), seed, region=k, sprinkle=False)
            yield ('samples', k, estimator), cube, filled, dict(estimator=estimator), mask
        seed += 1
        cube, filled, mask = make_case(2, ONE_PIXEL_PLANE, seed, sprinkle=False)
        yield ('one pixel', estimator), cube, filled, dict(
            estimator=estimator, border=2, pool_polarizations=False), mask


# ---- the independent statement -------------------------------------------------------------------
def _middle(values):
    """np.sort of the values, the two middle elements, float32 arithmetic: (median, whether a zero of
    either sign is among the middle pair)."""
    ordered = np.sort(values)
    n = len(ordered)
    lo, hi = ordered[(n - 1) // 2], ordered[n // 2]
    with np.errstate(all='ignore'):
        return np.float32(np.float32(lo + hi) / np.float32(2)), bool(lo == 0 or hi == 0)


def independent(cube, filled, first, stop, estimator, border, pool, region):
    """Per group of the contract: ``{field: [C][G]}`` and ``exact``, bool [C][G] per float field:
    whether the statement's value is to be met by bits (no zero of either sign where np.sort's order
    of -0 and +0 could show) or by ``==``."""
    C, P, H, W = cube.shape
    G = 1 if pool else P
    out = {name: np.full((C, G), np.nan, np.float32) for name in FIELDS[1:]}
    out['count'] = np.zeros((C, G), np.uint32)
    exact = {name: np.ones((C, G), bool) for name in FIELDS[1:]}
    constant = np.float32(1.4826022185056031)
    for c in range(first, stop):
        if not filled[c]:
            continue
        for g in range(G):
            planes = cube[c] if pool else cube[c, g:g + 1]
            inner = planes[:, border:H - border, border:W - border]
            if region is not None:
                inner = inner[:, region[border:H - border, border:W - border] != 0]
            x = inner[np.isfinite(inner)].astype(np.float32)
            out['count'][c, g] = x.size
            if not x.size:
                continue
            out['min'][c, g], out['max'][c, g] = x.min(), x.max()
            exact['min'][c, g], exact['max'][c, g] = x.min() != 0, x.max() != 0
            m, zero = _middle(x)
            out['median'][c, g] = m
            exact['median'][c, g] = not zero
            with np.errstate(all='ignore'):
                spread = np.abs(x) if estimator == 'median_abs' else np.abs((x - m).astype(np.float32))
                out['sigma'][c, g] = np.float32(_middle(spread)[0] * constant)
    return out, exact


# ---- the device runs (nothing of the package is imported until one is made) --------------------------

#: (pad of the channel pitch, offset of the view into the buffer), in floats
LAYOUTS = ((0, 0), (3, 0), (4, 0), (0, 1))
SENTINEL = SENTINELS[np.dtype(np.float32)]


def form(plane, pad, offset):
    """What kimg_cube_stats picks for a cube in a 16-byte aligned buffer."""
    M = int(np.prod(plane))
    return 'vector' if offset % 4 == 0 and (M + pad) % 4 == 0 and plane[2] % 4 == 0 else 'scalar'


class PaddedCube:
    """[C][P][H][W] inside a flat device buffer of sentinels: `offset` floats in, channel pitch
    P * H * W + pad."""

    def __init__(self, ctx, q, inner, pad, offset):
        from katsdpimager_amd import accel
        shape = inner.shape
        C, M = shape[0], int(np.prod(shape[1:]))
        pitch = M + pad
        self.host = np.full(offset + C * pitch, SENTINEL, np.float32)
        self.host[offset:].reshape(C, pitch)[:, :M] = inner.reshape(C, M)
        self.whole = accel.DeviceArray(ctx, self.host.shape, np.float32)
        self.whole.set(q, self.host)
        view = self.whole.tensor[offset:].view(C, pitch)[:, :M].unflatten(1, shape[1:])
        self.array = accel.DeviceArray(ctx, shape, np.float32, tensor=view)

    def assert_unchanged(self, q):
        assert np.array_equal(self.whole.get(q).view(np.uint32), self.host.view(np.uint32)), \
            'the cube or its padding changed'


def check(ctx, q, cube, filled, keywords, region, forms, where, layouts=LAYOUTS, device_region=False):
    """One case on the layouts against the twin; returns the twin's result."""
    from katsdpimager_amd import accel, cube_stats
    params = cube_stats.CubeStatsParameters(**keywords)
    twin = cube_stats.cube_stats_host(cube, filled, params, region)
    op = cube_stats.CubeStatsTemplate(ctx, params).instantiate(q, cube.shape)
    if device_region and region is not None:
        on_device = accel.DeviceArray(ctx, region.shape, np.uint8)
        on_device.set(q, region)
        region = on_device
    for pad, offset in layouts:
        source = PaddedCube(ctx, q, cube, pad, offset)
        forms.add(form(cube.shape[1:], pad, offset))
        got = op(source.array, filled=filled, region=region)
        source.assert_unchanged(q)
        assert_same(got, twin, where + (pad, offset))
    return twin


def assert_same(result, want, where=None):
    """Two results, all five outputs by bits."""
    for name in FIELDS:
        a, b = getattr(result, name), getattr(want, name)
        assert a.dtype == b.dtype and a.shape == b.shape, (where, name)
        different = a.view(np.uint32) != b.view(np.uint32)
        assert not different.any(), (where, name, np.argwhere(different)[:4].tolist(),
                                     a[different][:4].tolist(), b[different][:4].tolist())
