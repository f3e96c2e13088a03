"""CLEAN auto-masks (include/kimg.h, "CLEAN auto-masks"; katsdpimager_amd/mask.py): the clean mask
built on the device from the residual.  The reference has no masks, so the truth is a numpy
RESTATEMENT in this module:

* threshold: the CLEAN metric in float64 from the float32 pixels, compared strictly;
* dilation: the brute-force union of the plane shifted by every offset of the disk -- and the chord
  form (a pixel is set where some |dy| <= r has a set pixel within chord(dy) columns in row y + dy),
  proved equal to the brute force on the CPU for radius 0 to 8 and used for the large radii.

Thresholds on random float data are the midpoint between two adjacent sorted metric values, so that
no rounding of the kernel's float32 metric can flip a pixel; the boundary cases (metric ==
threshold, zeros, threshold 0) use small-integer images, where every evaluation order is exact.
All comparisons are exact equality of byte planes.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import golden_inputs as gi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
FILL = 0xAA                 # what every device plane holds before a call: padding must keep it


# ---- the truth ---------------------------------------------------------------------------------
def metric64(image, mode):
    """CLEAN metric in float64 from float32 pixels [P][H][W]."""
    wide = image.astype(np.float64)
    return np.abs(wide[0]) if mode == 0 else np.sum(wide * wide, axis=0)


def inside(shape, border):
    H, W = shape
    ok = np.zeros((H, W), bool)
    if H > 2 * border and W > 2 * border:
        ok[border:H - border, border:W - border] = True
    return ok


def threshold_truth(image, mode, border, threshold):
    with np.errstate(invalid='ignore'):
        return (inside(image.shape[1:], border) & (metric64(image, mode) > np.float64(threshold))).astype(np.uint8)


def shifted(plane, dy, dx):
    """out[y][x] = plane[y + dy][x + dx], False outside."""
    H, W = plane.shape
    out = np.zeros_like(plane)
    if abs(dy) >= H or abs(dx) >= W:
        return out
    ys, yd = slice(max(0, dy), min(H, H + dy)), slice(max(0, -dy), min(H, H - dy))
    xs, xd = slice(max(0, dx), min(W, W + dx)), slice(max(0, -dx), min(W, W - dx))
    out[yd, xd] = plane[ys, xs]
    return out


def dilate_brute(plane, radius):
    plane = np.asarray(plane) != 0
    out = np.zeros_like(plane)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            if dy * dy + dx * dx <= radius * radius:
                out |= shifted(plane, dy, dx)
    return out


def chord(radius, dy):
    """Largest c with c^2 + dy^2 <= radius^2."""
    c = 0
    while (c + 1) ** 2 + dy * dy <= radius * radius:
        c += 1
    return c


def dilate_chords(plane, radius):
    plane = np.asarray(plane) != 0
    H, W = plane.shape
    # set pixels in columns [x - c, x + c] of a row, from the row's running count
    running = np.concatenate([np.zeros((H, 1), np.int64), np.cumsum(plane, axis=1)], axis=1)
    x = np.arange(W)
    out = np.zeros_like(plane)
    for dy in range(-radius, radius + 1):
        c = chord(radius, abs(dy))
        near = running[:, np.minimum(x + c + 1, W)] - running[:, np.maximum(x - c, 0)] > 0
        out |= shifted(near, dy, 0)
    return out


def combine(dilated, or_with, and_with):
    out = dilated.copy()
    if or_with is not None:
        out |= or_with != 0
    if and_with is not None:
        out &= and_with != 0
    return out.astype(np.uint8)


# ---- CPU ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('radius', range(9))
def test_chord_form_is_the_brute_force(radius):
    rs = np.random.RandomState(radius)
    for density in (0.01, 0.1, 0.5):
        plane = rs.uniform(size=(40, 40)) < density
        np.testing.assert_array_equal(dilate_chords(plane, radius), dilate_brute(plane, radius))
    single = np.zeros((40, 40), bool)
    single[0, 39] = True
    np.testing.assert_array_equal(dilate_chords(single, radius), dilate_brute(single, radius))
    yy, xx = np.mgrid[:40, :40]
    np.testing.assert_array_equal(dilate_brute(single, radius), yy ** 2 + (xx - 39) ** 2 <= radius ** 2)


AUTO_SYMBOLS = ('kimg_mask_threshold', 'kimg_mask_dilate')


def test_auto_mask_symbols_declared_exported_prototyped():
    from katsdpimager_amd import _lib, build, mask
    build.build_lib()
    header = open(os.path.join(ROOT, 'include', 'kimg.h')).read()
    declared = set(re.findall(r'\b(kimg_[a-z0-9_]+)\s*\(', header))
    handle = _lib.lib()
    for name in AUTO_SYMBOLS:
        assert name in declared, name
        assert hasattr(handle, name), name
        assert _lib.PROTOTYPES[name][0] is ctypes.c_int
    assert len(_lib.PROTOTYPES['kimg_mask_threshold'][1]) == 12
    assert len(_lib.PROTOTYPES['kimg_mask_dilate'][1]) == 13
    assert int(re.search(r'#define KIMG_MASK_MAX_RADIUS (\d+)', header).group(1)) == mask.MAX_RADIUS == 64
    assert 'mask.hip' in build.SOURCES
    assert handle.kimg_version() == _lib.VERSION == 5


def test_argument_errors_without_gpu():
    """Decided before any HIP call (there is no GPU here; the pointers are not device memory)."""
    from katsdpimager_amd import _lib
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)
    q, r, s = p + 16384, p + 32768, p + 49152
    EINVAL = -10001

    def dilate(radius=3, src=p, dest=q, or_with=r, and_with=s, stride=64, count=None):
        return lib.kimg_mask_dilate(src, stride, dest, 64, 64, 64, radius, or_with, 64, and_with, 64,
                                    count, None)
    assert dilate(radius=-1) == EINVAL
    assert dilate(radius=65) == EINVAL
    assert dilate(stride=63) == EINVAL
    assert dilate(src=q) == EINVAL                      # in == out
    assert dilate(and_with=q) == EINVAL                 # and_with == out
    assert dilate(src=None) == EINVAL and dilate(dest=None) == EINVAL
    assert lib.kimg_mask_dilate(p, 64, q, 63, 64, 64, 3, None, 0, None, 0, None, None) == EINVAL
    assert lib.kimg_mask_dilate(p, 64, q, 64, 64, 64, 3, r, 63, None, 0, None, None) == EINVAL
    assert lib.kimg_mask_dilate(p, 64, q, 64, 64, 64, 3, None, 0, s, 63, None, None) == EINVAL
    assert lib.kimg_mask_dilate(p, 64, q, 64, 0, 64, 3, None, 0, None, 0, None, None) == EINVAL

    def threshold(P=1, mode=0, stride=64, mask_stride=64, border=2, image=p, mask=q):
        return lib.kimg_mask_threshold(image, stride, 64 * 64, 64, 64, P, border, mode, 1.0, mask,
                                       mask_stride, None)
    assert threshold(P=0) == EINVAL and threshold(P=5) == EINVAL
    assert threshold(mode=2) == EINVAL and threshold(mode=-1) == EINVAL
    assert threshold(mask_stride=63) == EINVAL and threshold(stride=63) == EINVAL
    assert threshold(border=-1) == EINVAL
    assert threshold(image=None) == EINVAL and threshold(mask=None) == EINVAL


def test_auto_mask_parameters():
    from katsdpimager_amd import mask
    p = mask.AutoMaskParameters(5, 3)
    assert (p.sigma, p.radius, p.cumulative) == (5.0, 3, True)
    assert mask.AutoMaskParameters(0.5, 0, cumulative=False).cumulative is False
    assert mask.AutoMaskParameters(1e6, 64).radius == 64
    for bad in ((0, 3), (-1, 3), (float('nan'), 3), (5, -1), (5, 65), (5, 2.5), ('five', 3), (5, None)):
        with pytest.raises(ValueError):
            mask.AutoMaskParameters(*bad)


def test_process_channel_accepts_auto_mask():
    from katsdpimager_amd import frontend, imaging
    params = list(inspect.signature(frontend.process_channel).parameters.values())
    assert params[-1].name == 'auto_mask' and params[-1].default is None
    for name in ('auto_mask', 'auto_mask_reset', 'auto_mask_counts'):
        assert callable(getattr(imaging.Imaging, name))


def test_fake_imager_sees_auto_mask_only_when_asked():
    """auto_mask=None: the driver makes the calls it made (no auto_mask call, no mask looked at);
    with parameters: one reset, and the mask of every major cycle between its noise estimate and
    its clean_reset."""
    from test_host_logic import _Recorder, _HostReader, _driver_params
    from katsdpimager_amd import frontend, mask, weight
    image_p, grid_p, clean_p = _driver_params()

    def drive(**kwargs):
        im = _Recorder(peaks=[1.0, 1.0], cycles_before_threshold=3)
        frontend.process_channel(_HostReader([5, 0, 3]), 0, im, image_p, grid_p, clean_p,
                                 weight.WeightType.UNIFORM, 4, 2, True, batched_clean=False, **kwargs)
        return [c[0] for c in im.calls]
    plain = drive()
    assert plain == drive(auto_mask=None)
    assert not any('mask' in name for name in plain)
    names = drive(auto_mask=mask.AutoMaskParameters(5, 3))
    assert names.count('auto_mask_reset') == 1 and names.count('auto_mask') == 2
    assert names.index('auto_mask_reset') < names.index('auto_mask')
    for i, name in enumerate(names):
        if name == 'auto_mask':
            assert names[i - 1] == 'noise_est' and names[i + 1] == 'clean_reset'
    assert names[-1] == 'set_clean_mask'                # (the mask of entry is given back)
    assert [n for n in names if 'mask' not in n] == plain


# ---- GPU: device planes with padding ---------------------------------------------------------------
class Plane:
    """A byte plane [H][W] inside a flat device buffer: ``offset`` bytes in, ``stride`` bytes between
    rows, every byte FILL before ``data`` goes in."""

    def __init__(self, q, shape, stride=None, offset=0, data=None, itemsize=1, planes=1):
        from katsdpimager_amd import accel
        self.q, self.shape = q, shape
        H, W = shape
        self.stride = W if stride is None else stride
        self.offset, self.itemsize, self.planes = offset, itemsize, planes
        self.plane_stride = H * self.stride
        self.host = np.full(offset + planes * self.plane_stride, FILL, np.uint8).repeat(itemsize)
        self.device = accel.DeviceArray(q.context, self.host.shape, np.uint8, queue=q)
        if data is not None:
            self.view(self.host)[...] = data
        self.device.set(q, self.host)

    def view(self, flat):
        """[planes][H][W] view of the payload of a flat byte array like the buffer."""
        H, W = self.shape
        items = flat.view(np.uint8 if self.itemsize == 1 else np.float32)[self.offset:]
        rows = items.reshape(self.planes, H, self.stride)[:, :, :W]
        return rows[0] if self.planes == 1 else rows

    @property
    def ptr(self):
        return self.device.ptr + self.offset * self.itemsize

    def get(self):
        """(payload, were the bytes outside it left alone?)"""
        flat = self.device.get(self.q)
        payload = self.view(flat).copy()
        rest = flat.copy()
        self.view(rest)[...] = self.view(self.host)
        return payload, np.array_equal(rest, self.host)


def queue():
    from helpers import context_queue
    return context_queue()[1]


# ---- GPU: kimg_mask_threshold ------------------------------------------------------------------------
def midpoint_threshold(values, quantile):
    """Midpoint between two adjacent sorted values near the quantile, where they lie well apart."""
    s = np.sort(values[np.isfinite(values)])
    if len(s) < 2:
        return np.float32(s[0] / 2 if len(s) else 0.5)
    i = min(int(quantile * len(s)), len(s) - 2)
    lo = max(0, i - 8)
    i = lo + int(np.argmax(np.diff(s[lo:i + 9])))
    thr = np.float32((s[i] + s[i + 1]) / 2)
    # (float32 rounding of the kernel's metric moves a value by 2^-22 of itself at the most)
    assert s[i] * (1 + 1e-6) < thr < s[i + 1] * (1 - 1e-6)
    return thr


THRESHOLD_SHAPES = [(1, 64, 64, 0, 0, 0), (4, 67, 131, 5, 3, 0), (2, 5, 3, 0, 0, 0), (1, 1, 1, 0, 0, 0),
                    (3, 33, 70, 2, 1, 3)]          # P, H, W, image row padding, mask row padding, offsets


@gpu
@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('border', [0, 3])
@pytest.mark.parametrize('P,H,W,ipad,mpad,off', THRESHOLD_SHAPES)
def test_mask_threshold(P, H, W, ipad, mpad, off, border, mode):
    from katsdpimager_amd import _lib
    lib, q = _lib.lib(), queue()
    rs = np.random.RandomState(P * 1000 + H + border)
    floats = rs.standard_normal((P, H, W)).astype(np.float32)
    with_nan = floats.copy()
    with_nan[0, H // 2, W // 2] = np.nan
    with_nan[P - 1, H // 3, W // 3] = np.nan
    integers = rs.randint(-3, 4, size=(P, H, W)).astype(np.float32)
    integers[:, ::2, ::3] = 0
    ok = inside((H, W), border)
    quantile = midpoint_threshold(metric64(floats, mode)[ok], 0.9)
    cases = [(floats, quantile), (with_nan, quantile), (with_nan, -1.0), (integers, 0.0),
             (integers, 4.0), (integers, 1.0), (floats, -1.0), (floats, np.inf), (floats, np.nan),
             (integers, -0.0)]
    for image, threshold in cases:
        want = threshold_truth(image, mode, border, threshold)
        src = Plane(q, (H, W), W + ipad, off, image, itemsize=4, planes=P)
        dst = Plane(q, (H, W), W + mpad, off)
        rc = lib.kimg_mask_threshold(src.ptr, src.stride, src.plane_stride, W, H, P, border, mode,
                                     float(threshold), dst.ptr, dst.stride, q.handle)
        assert rc == 0
        got, untouched = dst.get()
        assert untouched                                        # padding and offset bytes keep FILL
        assert set(np.unique(got)) <= {0, 1}
        np.testing.assert_array_equal(got, want)
        if threshold == -1.0 and image is floats:
            np.testing.assert_array_equal(got, ok.astype(np.uint8))     # all ones inside the border
        if not threshold < np.inf:
            assert not got.any()


# ---- GPU: kimg_mask_dilate ---------------------------------------------------------------------------
DILATE_PLANES = [(64, 64), (65, 130), (200, 131), (3, 300), (1, 1)]
RADII = [0, 1, 2, 5, 16, 17, 63, 64]


def dilate_inputs(H, W, rs):
    def single(*spots):
        plane = np.zeros((H, W), np.uint8)
        for y, x in spots:
            plane[y, x] = 1
        return plane
    inputs = {
        'centre': single((H // 2, W // 2)),
        'corner00': single((0, 0)), 'corner01': single((0, W - 1)),
        'corner10': single((H - 1, 0)), 'corner11': single((H - 1, W - 1)),
        'random1': (rs.uniform(size=(H, W)) < 0.01).astype(np.uint8),
        'random50': (rs.uniform(size=(H, W)) < 0.5).astype(np.uint8),
        'zeros': np.zeros((H, W), np.uint8),
        'ones': np.ones((H, W), np.uint8),
        'bytes': (rs.uniform(size=(H, W)) < 0.01).astype(np.uint8) * rs.choice([7, 255], size=(H, W)).astype(np.uint8),
    }
    for y, x in ((63, 63), (64, 64)):                           # the tile seam
        if y < H and x < W:
            inputs['seam%d' % y] = single((y, x))
    return inputs


@gpu
@pytest.mark.parametrize('radius', RADII)
@pytest.mark.parametrize('H,W', DILATE_PLANES)
def test_mask_dilate(H, W, radius):
    from katsdpimager_amd import _lib, accel
    lib, q = _lib.lib(), queue()
    rs = np.random.RandomState(H * 7 + W + radius)
    or_mask = (rs.uniform(size=(H, W)) < 0.05).astype(np.uint8) * 3
    and_mask = (rs.uniform(size=(H, W)) < 0.7).astype(np.uint8) * 200
    count = accel.DeviceArray(q.context, (1,), np.uint32, queue=q)
    layouts = [dict(src=(0, 0), dst=(0, 0), orw=(0, 0), andw=(0, 0)),                 # packed
               dict(src=(3, 1), dst=(5, 2), orw=(1, 3), andw=(4, 0))]                 # (row padding, offset)
    for name, plane in dilate_inputs(H, W, rs).items():
        dilated = dilate_brute(plane, radius) if radius <= 5 else dilate_chords(plane, radius)
        if name in ('centre', 'seam63', 'seam64') or name.startswith('corner'):
            (y,), (x,) = np.nonzero(plane)
            yy, xx = np.mgrid[:H, :W]
            np.testing.assert_array_equal(dilated, (yy - y) ** 2 + (xx - x) ** 2 <= radius * radius)
        for layout in layouts:
            def make(key, data=None):
                pad, off = layout[key]
                return Plane(q, (H, W), W + pad, off, data)
            src, orw, andw = make('src', plane), make('orw', or_mask), make('andw', and_mask)
            for use_or in (None, 'plane', 'out'):
                for use_and in (False, True):
                    want = combine(dilated, or_mask if use_or else None, and_mask if use_and else None)
                    dst = make('dst', or_mask if use_or == 'out' else None)
                    or_plane = {None: None, 'plane': orw, 'out': dst}[use_or]
                    rc = lib.kimg_mask_dilate(
                        src.ptr, src.stride, dst.ptr, dst.stride, W, H, radius,
                        or_plane.ptr if or_plane else None, or_plane.stride if or_plane else 0,
                        andw.ptr if use_and else None, andw.stride, count.ptr, q.handle)
                    assert rc == 0
                    got, untouched = dst.get()
                    assert untouched, (name, layout, use_or, use_and)
                    np.testing.assert_array_equal(got, want, err_msg=str((name, layout, use_or, use_and)))
                    # (the same counter call after call: the call's zeroing is part of the result)
                    assert int(count.get(q)[0]) == int(want.sum())
            for other in (src, orw, andw):                      # (read only)
                payload, untouched = other.get()
                assert untouched and np.array_equal(payload, other.view(other.host))
    # without a counter
    dst = Plane(q, (H, W))
    src = Plane(q, (H, W), data=plane)
    assert lib.kimg_mask_dilate(src.ptr, W, dst.ptr, W, W, H, radius, None, 0, None, 0, None, q.handle) == 0
    np.testing.assert_array_equal(dst.get()[0], dilated.astype(np.uint8))


@gpu
def test_pitch_below_width_is_refused_and_nothing_runs():
    """Each pitch of the two calls in turn one below the width: KIMG_EINVAL, and every buffer of the
    call -- sentinels inside and in the padding -- comes back bit for bit."""
    import torch
    from katsdpimager_amd import _lib, accel
    lib, q = _lib.lib(), queue()
    H = W = 64
    image = Plane(q, (H, W), W + 3, 1, itemsize=4, planes=2)
    planes = [Plane(q, (H, W), W + 3, 1) for _ in range(4)]
    count = accel.DeviceArray(q.context, (1,), np.uint32, queue=q)
    count.set(q, np.array([0xAAAAAAAA], np.uint32))
    q.finish()
    src, dst, orw, andw = planes

    def threshold(row=W + 3, mask_row=W + 3):
        return lib.kimg_mask_threshold(image.ptr, row, image.plane_stride, W, H, 2, 2, 1, 0.5, dst.ptr,
                                       mask_row, q.handle)

    def dilate(a=W + 3, b=W + 3, c=W + 3, d=W + 3):
        return lib.kimg_mask_dilate(src.ptr, a, dst.ptr, b, W, H, 3, orw.ptr, c, andw.ptr, d, count.ptr,
                                    q.handle)
    calls = [lambda: threshold(row=W - 1), lambda: threshold(mask_row=W - 1), lambda: dilate(a=W - 1),
             lambda: dilate(b=W - 1), lambda: dilate(c=W - 1), lambda: dilate(d=W - 1)]
    for call in calls:
        assert call() == -10001
        torch.cuda.synchronize()
        for plane in planes + [image]:
            assert np.array_equal(plane.device.get(q), plane.host)
        assert count.get(q)[0] == 0xAAAAAAAA
    assert threshold() == 0 and dilate() == 0               # (the same calls with the pitches right)


@gpu
def test_mask_operations():
    """The accel operators on the kernels: slots, the optional terms, the count slot's index."""
    from katsdpimager_amd import accel, mask
    from helpers import context_queue
    ctx, q = context_queue()
    rs = np.random.RandomState(5)
    image = rs.standard_normal((2, 70, 90)).astype(np.float32)
    threshold = midpoint_threshold(metric64(image, 1)[inside((70, 90), 7)], 0.95)
    op = mask.MaskThresholdTemplate(ctx, np.float32, 2, 1).instantiate(q, image.shape, 0.1)
    assert op.border_pixels == 7
    op.ensure_all_bound()
    op.buffer('image').set(q, image)
    op(threshold)
    seed = op.buffer('mask').get(q)
    np.testing.assert_array_equal(seed, threshold_truth(image, 1, 7, threshold))
    dil = mask.MaskDilateTemplate(ctx).instantiate(q, (70, 90), counts=3)
    dil.bind(src=op.buffer('mask'))
    dil.ensure_all_bound()
    assert dil.buffer('accumulate') is None and dil.buffer('restrict') is None
    dil.buffer('count').set(q, np.array([9, 9, 9], np.uint32))
    dil(4, 1)
    first = dil.buffer('dest').get(q)
    np.testing.assert_array_equal(first, dilate_brute(seed, 4))
    other = rs.uniform(size=(70, 90)) < 0.3
    restrict = accel.DeviceArray(ctx, (70, 90), np.uint8, queue=q)
    restrict.set(q, other.astype(np.uint8))
    op(np.float32(threshold * 0.5))
    seed2 = op.buffer('mask').get(q)
    dil(2, 2, accumulate=dil.buffer('dest'), restrict=restrict)
    want = combine(dilate_brute(seed2, 2), first, other)
    np.testing.assert_array_equal(dil.buffer('dest').get(q), want)
    np.testing.assert_array_equal(dil.buffer('count').get(q), [9, first.sum(), want.sum()])
    with pytest.raises(ValueError):
        dil(2, 3)
    with pytest.raises(ValueError):
        mask.MaskThresholdTemplate(ctx, np.float64, 2, 1)


# ---- GPU: the imager -----------------------------------------------------------------------------------
def metric32(image, mode):
    """The kernel's own arithmetic (clean_metric of clean.hip; MaskedClean._metric): float32, the
    squares and sums rounded one by one in polarization order."""
    if mode == 0:
        return np.abs(image[0])
    value = np.zeros(image.shape[1:], np.float32)
    for pol in range(image.shape[0]):
        value = value + image[pol] * image[pol]
    return value


def make_imager(P, mode, major=2):
    from helpers import context_queue, make_params
    from katsdpimager_amd import imaging, parameters, weight
    import test_clean_mask as tcm
    ctx, q = context_queue()
    c = dict(gi.E2E_CONFIGS['degrid'], P=P, mode=mode)
    assert c['pixels'] == tcm.G and c['border'] == tcm.BORDER
    ip, gp, ap = make_params(c)
    wp = parameters.WeightParameters(weight.WeightType(c['weight_type']), c['robustness'])
    cp = parameters.CleanParameters(1000, 0.1, 0.85, 5.0, mode, 0.01, 0.5, tcm.BORDER)
    im = imaging.ImagingTemplate(ctx, ap, ip.fixed, wp, gp.fixed, cp).instantiate(
        q, ip, gp, c['vis_block'], 0, major)
    im.ensure_all_bound()
    return im, q


@gpu
@pytest.mark.parametrize('mode,P', [(0, 1), (1, 1), (0, 4), (1, 4), (1, 3), (0, 2)])
def test_imaging_auto_mask(mode, P):
    """Imaging.auto_mask on the 256^2 problem of test_clean_mask: the restated mask exactly, and 200
    masked cycles under it that are MaskedClean's on the numpy mask, bit for bit."""
    import test_clean_mask as tcm
    from katsdpimager_amd import clean, mask
    psf, dirty = tcm.problem(mode, P)
    patch = (P,) + tcm.PATCH
    im, q = make_imager(P, mode)
    im.set_buffer('psf', psf)
    im.set_buffer('dirty', dirty)
    im.clear_model()
    noise = im.noise_est()
    params = mask.AutoMaskParameters(5, 3)
    im.auto_mask_reset()
    device = im.auto_mask(noise, params)
    assert im.clean_mask is device
    threshold = np.float32(clean.power_to_metric(mode, noise * clean.noise_threshold_scale(mode, 5, P)))
    bp = round(tcm.BORDER * tcm.G)
    seed = inside((tcm.G, tcm.G), bp) & (metric32(dirty, mode) > threshold)
    assert 10 < seed.sum() < seed.size // 4                     # (sources, not noise, not everything)
    # (no pixel sits where the float64 metric and the kernel's float32 metric could disagree)
    np.testing.assert_array_equal(seed, threshold_truth(dirty, mode, bp, threshold))
    want_mask = dilate_brute(seed, 3).astype(np.uint8)
    got_mask = device.get(q)
    np.testing.assert_array_equal(got_mask, want_mask)
    assert im.auto_mask_counts() == [int(want_mask.sum())]
    want = tcm.masked_run(tcm.G, tcm.BORDER, 0.1, mode, dirty, psf, patch, 0.0, tcm.CYCLES, want_mask)
    assert len(want[0]) == tcm.CYCLES
    im.clean_reset()
    values = im.clean_cycles(patch, 0.0, tcm.CYCLES)
    assert values == [float(v) for v, _, _ in want[0]]
    np.testing.assert_array_equal(im.get_buffer('dirty'), want[1])
    np.testing.assert_array_equal(im.get_buffer('model'), want[2])
    np.testing.assert_array_equal(im.get_buffer('tile_max'), want[3])
    np.testing.assert_array_equal(im.get_buffer('tile_pos'), want[4])
    assert sorted(im._model_components) == sorted({pos for _, pos, _ in want[0]})
    # the next call: cumulative joins the masks, a restriction cuts them, a reset starts over
    residual = im.get_buffer('dirty')
    seed2 = inside((tcm.G, tcm.G), bp) & (metric32(residual, mode) > threshold)
    left = np.zeros((tcm.G, tcm.G), np.uint8)
    left[:, :tcm.G // 2] = 1
    second = im.auto_mask(noise, params, restrict=left)
    assert second is device
    joined = combine(dilate_brute(seed2, 3), want_mask, left)
    np.testing.assert_array_equal(second.get(q), joined)
    # the auto mask as its own restriction (what clean_mask is now): copied, not cut in place
    assert im.clean_mask is device
    third = im.auto_mask(noise, params, restrict=im.clean_mask)
    np.testing.assert_array_equal(third.get(q), joined)
    im.auto_mask_reset()
    alone = im.auto_mask(noise, mask.AutoMaskParameters(5, 3, cumulative=False))
    np.testing.assert_array_equal(alone.get(q), dilate_brute(seed2, 3).astype(np.uint8))
    assert im.auto_mask_counts() == [int(dilate_brute(seed2, 3).sum())]
    im.set_clean_mask(None)
    assert im.clean_mask is None


# ---- GPU: the driver -------------------------------------------------------------------------------------
def drive(major, imager_mask=None, **kwargs):
    """frontend.process_channel on the G9 `degrid` channel (the recipe of
    test_clean_mask.test_process_channel_with_clean_mask) with a fresh imager."""
    import test_clean_mask as tcm
    from katsdpimager_amd import frontend, imaging
    c = gi.E2E_CONFIGS['degrid']
    ctx, q, ip, gp, ap, wp, cp, reader = tcm._channel(c)
    im = imaging.ImagingTemplate(ctx, ap, ip.fixed, wp, gp.fixed, cp).instantiate(
        q, ip, gp, c['vis_block'], 0, major)
    im.ensure_all_bound()
    if imager_mask is not None:
        im.set_clean_mask(imager_mask)
    entry = im.clean_mask
    stats = frontend.process_channel(reader, 0, im, ip, gp, cp, wp.weight_type, c['vis_block'],
                                     major, c['degrid'], **kwargs)
    assert im.clean_mask is entry                       # the imager has back the mask it had
    return stats, im.get_buffer('dirty'), im.get_buffer('model'), q


def support(model):
    return np.any(model != 0, axis=0)


@gpu
def test_driver_auto_mask_is_the_same_run_under_its_mask():
    from katsdpimager_amd import mask
    a, dirty_a, model_a, q = drive(1, auto_mask=mask.AutoMaskParameters(5, 3))
    plane = a['auto_mask'].get(q)
    assert set(np.unique(plane)) <= {0, 1} and 0 < plane.sum() < plane.size
    assert a['mask_pixels'] == [int(plane.sum())]
    assert a['minor'] > 0 and np.any(model_a)
    assert not np.any(support(model_a) & (plane == 0))
    b, dirty_b, model_b, q = drive(1, clean_mask=plane)
    assert 'auto_mask' not in b and 'mask_pixels' not in b
    print('A vs B: dirty max |diff| %.3e, model max |diff| %.3e, peaks %r %r, minor %d %d' % (
        np.max(np.abs(dirty_a - dirty_b)), np.max(np.abs(model_a - model_b)), a['peaks'], b['peaks'],
        a['minor'], b['minor']))
    assert a['peaks'] == b['peaks'] and a['minor'] == b['minor']
    np.testing.assert_array_equal(dirty_a, dirty_b)
    np.testing.assert_array_equal(model_a, model_b)


@gpu
def test_driver_cumulative_masks_grow():
    from katsdpimager_amd import mask
    out, dirty, model, q = drive(2, auto_mask=mask.AutoMaskParameters(5, 3))
    assert out['major'] == 2 and len(out['mask_pixels']) == 2
    assert out['mask_pixels'][0] <= out['mask_pixels'][1]
    plane = out['auto_mask'].get(q)
    assert out['mask_pixels'][1] == int(plane.sum())
    assert np.any(model) and not np.any(support(model) & (plane == 0))


@gpu
def test_driver_empty_auto_mask():
    from katsdpimager_amd import mask
    out, dirty, model, q = drive(2, auto_mask=mask.AutoMaskParameters(1e6, 3))
    assert not out['auto_mask'].get(q).any() and out['mask_pixels'] == [0]
    assert out['peaks'] == [] and out['minor'] == 0 and not np.any(model)


@gpu
def test_driver_user_mask_and_auto_mask_intersect():
    from katsdpimager_amd import mask
    pixels = gi.E2E_CONFIGS['degrid']['pixels']
    left = np.zeros((pixels, pixels), np.uint8)
    left[:, :pixels // 2] = 1
    params = mask.AutoMaskParameters(5, 3)
    free, _, free_model, q = drive(2, auto_mask=params)
    assert np.any(free_model[:, :, pixels // 2:])               # (there is flux to keep out)
    out, dirty, model, q = drive(2, clean_mask=left, auto_mask=params)
    plane = out['auto_mask'].get(q)
    assert np.any(model) and not np.any(model[:, :, pixels // 2:])
    assert not plane[:, pixels // 2:].any() and not np.any(support(model) & (plane == 0))
    # ... and the same with the mask set on the imager beforehand (drive() checks it is still there)
    again, dirty2, model2, q = drive(2, imager_mask=left, auto_mask=params)
    assert again['mask_pixels'] == out['mask_pixels']
    assert not np.any(model2[:, :, pixels // 2:])
