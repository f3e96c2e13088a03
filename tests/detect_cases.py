"""Shared by test_detect_host.py and test_detect_gpu.py: the five contracts of the detection mask
(include/kimg.h, "Detection mask") restated per voxel in plain Python loops -- Python floats for the
float64 sum, np.float32 scalars for the float32 product and compares, no code of the package --, the
cubes, masks and tables both suites run, and the ABI's argument errors."""
import ctypes
import math

import numpy as np

from helpers import SENTINELS

EINVAL = -10001
EUNSUPPORTED = -10002
POLARITIES = ('positive', 'negative', 'both')
ESTIMATORS = ('median_abs', 'mad')
WIDTHS = (1, 3, 7, 15, 31)
QUIET = np.array([0x7fc00000], np.uint32).view(np.float32)[0]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_bits(got, want, where=None):
    """uint32 patterns equal, NaN in the same places (any NaN pattern is a NaN); other dtypes equal."""
    assert got.shape == want.shape and got.dtype == want.dtype, where
    if got.dtype == np.float32:
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), where
        different = (bits(got) != bits(want)) & ~nan
        assert not different.any(), (where, np.argwhere(different)[:4].tolist(),
                                     got[different][:4].tolist(), want[different][:4].tolist())
    else:
        assert np.array_equal(got, want), (where, np.argwhere(got != want)[:4].tolist())


# ---- the contracts, per voxel ------------------------------------------------------------------------

def _finite(x):
    return not (math.isnan(x) or math.isinf(x))


def restate_boxcar(cube, filled, width, mask=None, blank=False):
    """[C][M] float32 -> [C][M]; NaN in the channels that are not filled (which the call leaves)."""
    C, M = cube.shape
    h = width // 2
    out = np.full((C, M), np.nan, np.float32)
    for j in range(M):
        for c in range(C):
            if not filled[c]:
                continue
            acc = 0.0
            for k in range(c - h, c + h + 1):
                z = 0.0
                if 0 <= k < C and filled[k] and _finite(float(cube[k, j])) \
                        and (mask is None or mask[k, j] == 0):
                    z = float(cube[k, j])
                acc = acc + z
            out[c, j] = np.float32(acc / float(width))
            if blank and not _finite(float(cube[c, j])):
                out[c, j] = QUIET
    return out


def restate_reblank(work, cube, filled):
    C, M = cube.shape
    out = work.copy()
    for c in range(C):
        for j in range(M):
            if filled[c] and not _finite(float(cube[c, j])):
                out[c, j] = QUIET
    return out


def restate_threshold(work, mask, filled, sigma, threshold, polarity):
    """work [C][P][N], mask uint8 [C][P][N], sigma float32 [C][G]."""
    C, P, N = work.shape
    G = sigma.shape[1]
    out = mask.copy()
    for c in range(C):
        if not filled[c]:
            continue
        for p in range(P):
            with np.errstate(all='ignore'):
                cut = np.float32(np.float32(threshold) * sigma[c, 0 if G == 1 else p])
            for j in range(N):
                s = np.float32(work[c, p, j])
                if not _finite(float(s)):
                    continue
                if polarity == 'positive':
                    over = s > cut
                elif polarity == 'negative':
                    over = np.float32(-s) > cut
                else:
                    over = np.float32(abs(s)) > cut
                if over:
                    out[c, p, j] = 1
    return out


def restate_prune(mask, min_channels):
    C, M = mask.shape
    out = np.zeros((C, M), np.uint8)
    for j in range(M):
        c = 0
        while c < C:
            if mask[c, j] == 0:
                c += 1
                continue
            end = c
            while end < C and mask[end, j] != 0:
                end += 1
            if end - c >= min_channels:
                out[c:end, j] = 1
            c = end
    return out


def restate_apply(cube, mask, filled, invert):
    C, M = cube.shape
    out = cube.copy()
    for c in range(C):
        for j in range(M):
            if filled[c]:
                out[c, j] = cube[c, j] if (mask[c, j] != 0) != bool(invert) else QUIET
    return out


# ---- cubes, masks, tables ----------------------------------------------------------------------------

def sprinkled_cube(C, plane, seed):
    """Unit noise about a level, with NaN, +Inf, -Inf, -0, +0 and denormals sprinkled in."""
    rng = np.random.default_rng(seed)
    shape = (C,) + tuple(plane)
    cube = rng.normal(0.5, 1.0, shape).astype(np.float32)
    pick = rng.random(shape)
    cube[pick < 0.10] = np.nan
    cube[(pick >= 0.10) & (pick < 0.12)] = np.inf
    cube[(pick >= 0.12) & (pick < 0.14)] = -np.inf
    cube[(pick >= 0.14) & (pick < 0.17)] = -0.0
    cube[(pick >= 0.17) & (pick < 0.19)] = 0.0
    cube[(pick >= 0.19) & (pick < 0.21)] = np.float32(1e-40)
    cube[(pick >= 0.21) & (pick < 0.23)] = np.float32(-3e-42)
    return cube


def filled_for(C, turn):
    """Unfilled channels at the first and last channel and in the middle, by turns more or fewer of
    them; a band of one channel is filled."""
    filled = np.ones(C, np.uint8)
    if C == 1:
        return filled
    for c in ((0, C - 1, C // 2), (C - 1,), (0, C // 2), (31, 32, 64, C // 2))[turn % 4]:
        if 0 <= c < C:
            filled[c] = 0
    if not filled.any():
        filled[C // 2] = 1
    return filled


def random_mask(shape, seed, density=0.3, values=(1,)):
    """uint8 mask with about `density` of its bytes set, to the values given (0 and 1 only unless
    asked: other nonzero values read as set)."""
    rng = np.random.default_rng(seed)
    mask = np.zeros(shape, np.uint8)
    on = rng.random(shape) < density
    mask[on] = rng.choice(np.asarray(values, np.uint8), int(on.sum()))
    return mask


def run_mask(C, M, seed):
    """A mask for prune: element j's column is made of runs whose lengths cycle through 1 .. 5 and C,
    at the start of the band, at its end and in between, some bytes 2 or 255 instead of 1; some
    columns are empty, some full."""
    rng = np.random.default_rng(seed)
    if M > 91:
        # (91 columns of their own, 13 of each kind, repeated along the plane)
        return np.ascontiguousarray(np.tile(run_mask(C, 91, seed), (1, M // 91 + 1))[:, :M])
    mask = np.zeros((C, M), np.uint8)
    for j in range(M):
        kind = j % 7
        if kind == 0:
            continue
        if kind == 1:
            mask[:, j] = 1
            continue
        c = 0 if kind % 2 else int(rng.integers(0, 3))
        while c < C:
            length = int(rng.integers(1, 6))
            mask[c:c + length, j] = rng.choice(np.array([1, 1, 1, 2, 255], np.uint8), min(length, C - c))
            c += length + int(rng.integers(1, 4))
        if kind == 6:
            mask[C - 1, j] = 1
    return mask


def sigma_table(C, G, seed):
    """float32 [C][G] around 1 with a NaN, a 0, a -0 and a negative entry where they fit."""
    rng = np.random.default_rng(seed)
    sigma = rng.uniform(0.2, 0.5, (C, G)).astype(np.float32)
    flat = sigma.reshape(-1)
    for i, value in zip(range(1, flat.size, 3), (np.nan, 0.0, -0.0, -0.25, np.inf)):
        flat[i] = value
    return sigma


# ---- the finder's cubes ------------------------------------------------------------------------------

def gaussian_source(shape, centre, fwhm_pixels, fwhm_channels, amplitude):
    """[C][1][H][W] float64: a source that is Gaussian in space and along the spectrum."""
    C, _, H, W = shape
    c0, y0, x0 = centre
    to_sigma = 1.0 / (2.0 * math.sqrt(2.0 * math.log(2.0)))
    sp, sc = fwhm_pixels * to_sigma, fwhm_channels * to_sigma
    c = np.arange(C, dtype=np.float64).reshape(C, 1, 1, 1)
    y = np.arange(H, dtype=np.float64).reshape(1, 1, H, 1)
    x = np.arange(W, dtype=np.float64).reshape(1, 1, 1, W)
    return amplitude * np.exp(-0.5 * (((y - y0) ** 2 + (x - x0) ** 2) / sp ** 2 + (c - c0) ** 2 / sc ** 2))


FINDER_SHAPE = (16, 2, 40, 48)
FINDER_UNFILLED = (0, 7, 15)


def finder_cube():
    """(cube, filled, region) of the finder's comparison: (16, 2, 40, 48), unit noise, a bright and a
    faint source in each polarization, three unfilled channels (the first, the last and one between)
    and a NaN corner."""
    rng = np.random.default_rng(20)
    C, P, H, W = FINDER_SHAPE
    cube = rng.normal(0.0, 1.0, FINDER_SHAPE)
    for p in range(P):
        one = (C, 1, H, W)
        cube[:, p:p + 1] += gaussian_source(one, (4 + 5 * p, 12, 14 + 10 * p), 3.0, 3.0, 9.0)
        cube[:, p:p + 1] += gaussian_source(one, (10 - 4 * p, 28, 30 - 8 * p), 5.0, 5.0, 2.5)
    cube = cube.astype(np.float32)
    cube[:, :, :6, :5] = np.nan
    cube[3, 1, 20, 20] = np.inf
    filled = np.ones(C, np.uint8)
    filled[list(FINDER_UNFILLED)] = 0
    region = np.ones((H, W), np.uint8)
    region[8:20, 8:40] = 0
    return cube, filled, region


#: the demonstration (16, 1, 48, 40): seeded unit Gaussian noise plus one source of FWHM 4 px x 5
#: channels whose peak lies below threshold x sigma.  Seed and amplitude were fixed on the CPU with the
#: twin (test_detect_host.py asserts what they were chosen for).
FAINT_SHAPE = (16, 1, 48, 40)
FAINT_CENTRE = (8, 24, 20)
FAINT_SEED = 7
FAINT_AMPLITUDE = 3.0
FAINT_THRESHOLD = 5.0


def faint_cube():
    rng = np.random.default_rng(FAINT_SEED)
    cube = rng.normal(0.0, 1.0, FAINT_SHAPE)
    cube += gaussian_source(FAINT_SHAPE, FAINT_CENTRE, 4.0, 5.0, FAINT_AMPLITUDE)
    return cube.astype(np.float32), np.ones(FAINT_SHAPE[0], np.uint8)


def assert_faint_source(single, full):
    """What the demonstration shows, on the masks of the per-voxel clip and of the full kernel set."""
    c0, y0, x0 = FAINT_CENTRE
    assert not single[c0 - 2:c0 + 3, 0, y0 - 4:y0 + 5, x0 - 4:x0 + 5].any(), 'the plain clip saw the source'
    assert full[c0, 0, y0, x0] == 1, 'the source is not detected'
    c, _, y, x = np.nonzero(full)
    near = (np.abs(c - c0) <= 5) & (np.abs(y - y0) <= 8) & (np.abs(x - x0) <= 8)
    assert near.all(), 'detections away from the source: {}'.format(
        list(zip(c[~near].tolist(), y[~near].tolist(), x[~near].tolist()))[:4])


# ---- the device buffers (nothing of the package is imported until one is made) -------------------------

FLOAT_LAYOUTS = ((0, 0), (3, 0), (4, 0), (0, 1))
MASK_LAYOUTS = ((0, 0), (1, 0), (4, 0), (0, 1), (3, 0))
FLOAT_SENTINEL = SENTINELS[np.dtype(np.float32)]
MASK_SENTINEL = np.uint8(0xa5)           # (nonzero: a read of the padding is a set voxel)


def float_form(M, pad, offset):
    if offset % 4 or (M + pad) % 4 or M < 4:
        return 'scalar'
    return 'vector' if M % 4 == 0 else 'vector+tail'


def mask_form(M, pad, offset):
    return 'bytes' if offset % 4 or (M + pad) % 4 else 'word'


class Padded:
    """[C][M] of float32 or uint8 inside a flat device buffer of sentinels: `offset` elements in,
    channel pitch M + pad.  `inner` None: sentinels throughout (a target)."""

    def __init__(self, ctx, q, C, M, inner, pad, offset, dtype=np.float32):
        from katsdpimager_amd import accel
        self.C, self.M, self.pitch, self.offset = C, M, M + pad, offset
        self.dtype = np.dtype(dtype)
        sentinel = FLOAT_SENTINEL if self.dtype == np.float32 else MASK_SENTINEL
        self.host = np.full(offset + C * self.pitch, sentinel, self.dtype)
        if inner is not None:
            self.rows(self.host)[:, :M] = inner.reshape(C, M)
        self.whole = accel.DeviceArray(ctx, self.host.shape, self.dtype)
        self.whole.set(q, self.host)
        self.ptr = self.whole.ptr + offset * self.dtype.itemsize

    def rows(self, flat):
        return flat[self.offset:].reshape(self.C, self.pitch)

    def assert_holds(self, q, want, channels, where):
        """The buffer holds `want` [C][M] in `channels` (a bool [C]; None: all) and what it held before
        everywhere else; returns nothing."""
        now = self.whole.get(q)
        expect = self.host.copy()
        on = np.ones(self.C, bool) if channels is None else np.asarray(channels) != 0
        self.rows(expect)[on, :self.M] = want.reshape(self.C, self.M)[on]
        assert_same_bits(now, expect, where)

    def assert_unchanged(self, q, where):
        assert np.array_equal(self.whole.get(q).view(np.uint8), self.host.view(np.uint8)), \
            (where, 'an input or its padding changed')


def host_ptr(array):
    return array.ctypes.data_as(ctypes.c_void_p)


# ---- the ABI's argument errors ---------------------------------------------------------------------

def abi_rejections(lib, cube, mask, out, sigma, filled, stream=None):
    """(name, code the call returned, code the header lists) for the rejections of the five entries.
    ``cube``, ``out``: pointers to float32 [4][16] with pitch 16; ``mask``: uint8 [4][16] with pitch
    16; ``sigma``: float32 [4]; ``filled``: host uint8 [4] as a pointer."""
    C, M = 4, 16
    P = ctypes.c_void_p
    inside = P(cube.value + 4 * 8)          # overlaps the cube without being it
    odd = P(cube.value + 2)                 # not 4-byte aligned
    nan, inf = float('nan'), float('inf')
    box = lib.kimg_cube_boxcar
    reb = lib.kimg_cube_reblank
    thr = lib.kimg_cube_threshold
    pru = lib.kimg_cube_mask_prune
    app = lib.kimg_cube_mask_apply
    calls = [
        ('boxcar ok', box(cube, M, mask, M, out, M, C, M, filled, 3, 0, stream), 0),
        ('boxcar ok without a mask', box(cube, M, None, 0, out, M, C, M, filled, 31, 1, stream), 0),
        ('boxcar null cube', box(None, M, mask, M, out, M, C, M, filled, 3, 0, stream), EINVAL),
        ('boxcar null out', box(cube, M, mask, M, None, M, C, M, filled, 3, 0, stream), EINVAL),
        ('boxcar null filled', box(cube, M, mask, M, out, M, C, M, None, 3, 0, stream), EINVAL),
        ('boxcar even width', box(cube, M, mask, M, out, M, C, M, filled, 2, 0, stream), EINVAL),
        ('boxcar width 0', box(cube, M, mask, M, out, M, C, M, filled, 0, 0, stream), EINVAL),
        ('boxcar width 33', box(cube, M, mask, M, out, M, C, M, filled, 33, 0, stream), EINVAL),
        ('boxcar in place', box(cube, M, mask, M, cube, M, C, M, filled, 3, 0, stream), EINVAL),
        ('boxcar overlap', box(cube, M, mask, M, inside, M, C, M, filled, 3, 0, stream), EINVAL),
        ('boxcar pitch', box(cube, M - 1, mask, M, out, M, C, M, filled, 3, 0, stream), EINVAL),
        ('boxcar out pitch', box(cube, M, mask, M, out, M - 1, C, M, filled, 3, 0, stream), EINVAL),
        ('boxcar mask pitch', box(cube, M, mask, M - 1, out, M, C, M, filled, 3, 0, stream), EINVAL),
        ('boxcar C 0', box(cube, M, mask, M, out, M, 0, M, filled, 3, 0, stream), EINVAL),
        ('boxcar M < 0', box(cube, M, mask, M, out, M, C, -1, filled, 3, 0, stream), EINVAL),
        ('boxcar misaligned', box(odd, M, mask, M, out, M, C, M, filled, 3, 0, stream), EINVAL),
        ('boxcar C 4097', box(cube, M, mask, M, out, M, 4097, M, filled, 3, 0, stream), EUNSUPPORTED),
        ('boxcar M 0', box(cube, M, mask, M, out, M, C, 0, filled, 3, 0, stream), 0),
        ('reblank ok', reb(out, M, cube, M, C, M, filled, stream), 0),
        ('reblank null work', reb(None, M, cube, M, C, M, filled, stream), EINVAL),
        ('reblank null cube', reb(out, M, None, M, C, M, filled, stream), EINVAL),
        ('reblank null filled', reb(out, M, cube, M, C, M, None, stream), EINVAL),
        ('reblank pitch', reb(out, M - 1, cube, M, C, M, filled, stream), EINVAL),
        ('reblank overlap', reb(inside, M, cube, M, C, M, filled, stream), EINVAL),
        ('reblank C 4097', reb(out, M, cube, M, 4097, M, filled, stream), EUNSUPPORTED),
        ('threshold ok', thr(cube, M, mask, M, C, 1, 4, 4, filled, sigma, 1, 5.0, 0, stream), 0),
        ('threshold null work', thr(None, M, mask, M, C, 1, 4, 4, filled, sigma, 1, 5.0, 0, stream), EINVAL),
        ('threshold null mask', thr(cube, M, None, M, C, 1, 4, 4, filled, sigma, 1, 5.0, 0, stream), EINVAL),
        ('threshold null sigma', thr(cube, M, mask, M, C, 1, 4, 4, filled, None, 1, 5.0, 0, stream), EINVAL),
        ('threshold null filled', thr(cube, M, mask, M, C, 1, 4, 4, None, sigma, 1, 5.0, 0, stream), EINVAL),
        ('threshold polarity 3', thr(cube, M, mask, M, C, 1, 4, 4, filled, sigma, 1, 5.0, 3, stream), EINVAL),
        ('threshold polarity -1', thr(cube, M, mask, M, C, 1, 4, 4, filled, sigma, 1, 5.0, -1, stream), EINVAL),
        ('threshold 0', thr(cube, M, mask, M, C, 1, 4, 4, filled, sigma, 1, 0.0, 0, stream), EINVAL),
        ('threshold < 0', thr(cube, M, mask, M, C, 1, 4, 4, filled, sigma, 1, -1.0, 0, stream), EINVAL),
        ('threshold NaN', thr(cube, M, mask, M, C, 1, 4, 4, filled, sigma, 1, nan, 0, stream), EINVAL),
        ('threshold Inf', thr(cube, M, mask, M, C, 1, 4, 4, filled, sigma, 1, inf, 0, stream), EINVAL),
        ('threshold groups 2 of 1', thr(cube, M, mask, M, C, 1, 4, 4, filled, sigma, 2, 5.0, 0, stream), EINVAL),
        ('threshold groups 0', thr(cube, M, mask, M, C, 2, 2, 4, filled, sigma, 0, 5.0, 0, stream), EINVAL),
        ('threshold pitch', thr(cube, M - 1, mask, M, C, 1, 4, 4, filled, sigma, 1, 5.0, 0, stream), EINVAL),
        ('threshold mask pitch', thr(cube, M, mask, M - 1, C, 1, 4, 4, filled, sigma, 1, 5.0, 0, stream), EINVAL),
        ('threshold H 0', thr(cube, M, mask, M, C, 1, 0, 4, filled, sigma, 1, 5.0, 0, stream), EINVAL),
        ('threshold C 4097', thr(cube, M, mask, M, 4097, 1, 4, 4, filled, sigma, 1, 5.0, 0, stream), EUNSUPPORTED),
        ('prune ok', pru(mask, M, C, M, 2, stream), 0),
        ('prune null', pru(None, M, C, M, 2, stream), EINVAL),
        ('prune min 0', pru(mask, M, C, M, 0, stream), EINVAL),
        ('prune min C + 1', pru(mask, M, C, M, C + 1, stream), EINVAL),
        ('prune pitch', pru(mask, M - 1, C, M, 2, stream), EINVAL),
        ('prune C 0', pru(mask, M, 0, M, 1, stream), EINVAL),
        ('prune C 4097', pru(mask, M, 4097, M, 2, stream), EUNSUPPORTED),
        ('apply ok out', app(cube, M, mask, M, out, M, C, M, filled, 0, stream), 0),
        ('apply ok in place', app(out, M, mask, M, out, M, C, M, filled, 1, stream), 0),
        ('apply null cube', app(None, M, mask, M, out, M, C, M, filled, 0, stream), EINVAL),
        ('apply null mask', app(cube, M, None, M, out, M, C, M, filled, 0, stream), EINVAL),
        ('apply null line', app(cube, M, mask, M, None, M, C, M, filled, 0, stream), EINVAL),
        ('apply null filled', app(cube, M, mask, M, out, M, C, M, None, 0, stream), EINVAL),
        ('apply overlap', app(cube, M, mask, M, inside, M, C, M, filled, 0, stream), EINVAL),
        ('apply same pointer, other pitch', app(cube, M + 4, mask, M, cube, M, C - 1, M, filled, 0, stream), EINVAL),
        ('apply pitch', app(cube, M - 1, mask, M, out, M, C, M, filled, 0, stream), EINVAL),
        ('apply mask pitch', app(cube, M, mask, M - 1, out, M, C, M, filled, 0, stream), EINVAL),
        ('apply C 4097', app(cube, M, mask, M, out, M, 4097, M, filled, 0, stream), EUNSUPPORTED),
    ]
    return calls
