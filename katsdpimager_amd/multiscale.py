"""Multi-scale CLEAN: Gaussian scales beside the Hogbom minor cycle.

An operator of its own next to :mod:`clean` (csrc/clean_scales.hip; include/kimg.h, "Multi-scale
CLEAN").  The reference has none.  Every scale k keeps its own residual R_k = dirty * t_k / n_k
(R_0 is the dirty image itself); a cycle takes the scale whose biased peak is largest and
subtracts the cross patches X_j,k from every R_j, so that nothing is ever re-convolved.  The
arithmetic is float32 in a fixed order: :class:`MultiScaleCleanHost` states it in numpy and
:class:`MultiScaleClean` matches it bit for bit; with the single scale 0 both take exactly the
components of the Hogbom path.
"""
import ctypes
import math

import numpy as np

from . import accel, types
from ._lib import lib, check
from .image_plane import (ImageTemplate, border_pixels, check_polarizations, plane_args,
                          plane_pitches)
from .parameters import CLEAN_I

TILE = 32
MAX_SCALES = 6          # KIMG_CLEAN_SCALES_MAX
MAX_RADIUS = 64         # KIMG_CLEAN_SCALES_MAX_RADIUS
_TAPS_PITCH = 192
_CROSS_PITCH = 320
_SETUP_PSF, _SETUP_RESIDUALS = 1, 2     # KIMG_CLEAN_SCALES_PSF, _RESIDUALS
_FWHM = 2.0 * math.sqrt(2.0 * math.log(2.0))


def scale_radius(scale):
    """Radius in pixels of the taps of a Gaussian of FWHM ``scale`` pixels: ceil(3 sigma)."""
    return int(math.ceil(3.0 * (scale / _FWHM))) if scale > 0 else 0


def _taps64(scale):
    R = scale_radius(scale)
    if R == 0:
        return np.ones(1, np.float64)
    sigma = scale / _FWHM
    i = np.arange(2 * R + 1, dtype=np.float64)
    t = np.exp(-(i - R) ** 2 / (2.0 * sigma * sigma))
    return t / t.sum()


def scale_taps(scale):
    """The 2 R + 1 taps of scale ``scale`` (FWHM in pixels; 0 = the delta): a Gaussian sampled in
    float64, divided by its sum and rounded once to float32."""
    return _taps64(scale).astype(np.float32)


def cross_taps(scale_j, scale_k):
    """Taps of scale j convolved with those of scale k, in float64 from the unrounded taps, rounded
    once: radius R_j + R_k."""
    return np.convolve(_taps64(scale_j), _taps64(scale_k)).astype(np.float32)


class MultiScaleParameters:
    """``scales``: Gaussian FWHMs in pixels, strictly ascending, the first one 0 (the delta), at
    most 6, none wider than radius 64.  ``biases``: one factor per scale that its peak is
    multiplied by when the scales are compared (default 1 - 0.6 scale / largest scale)."""

    def __init__(self, scales, biases=None):
        scales = [float(s) for s in scales]
        if not scales or scales[0] != 0.0:
            raise ValueError('the first scale must be 0 (the delta)')
        if len(scales) > MAX_SCALES:
            raise ValueError('at most {} scales'.format(MAX_SCALES))
        if any(b <= a for a, b in zip(scales, scales[1:])):
            raise ValueError('scales must be strictly ascending')
        self.scales = scales
        self.radii = [scale_radius(s) for s in scales]
        if max(self.radii) > MAX_RADIUS:
            raise ValueError('a scale of radius {} exceeds {}'.format(max(self.radii), MAX_RADIUS))
        if biases is None:
            largest = scales[-1]
            biases = [1.0 - 0.6 * s / largest if largest > 0 else 1.0 for s in scales]
        if len(biases) != len(scales):
            raise ValueError('one bias per scale')
        self.biases = np.array(biases, np.float64).astype(np.float32)
        self.taps = [scale_taps(s) for s in scales]
        self.cross = {(j, k): cross_taps(scales[j], scales[k])
                      for j in range(len(scales)) for k in range(j, len(scales))}

    def __len__(self):
        return len(self.scales)

    def cross_taps(self, j, k):
        return self.cross[(j, k) if j <= k else (k, j)]


def log_dtype(num_polarizations):
    return np.dtype([('scale', np.int32), ('y', np.int32), ('x', np.int32), ('peak', np.float32),
                     ('flux', np.float32, (num_polarizations,))])


def crop_range(n, patch, radius):
    """The centred box of patch + 2 radius pixels of an axis of n, clipped to it: (lo, hi)."""
    size = patch + 2 * radius
    start = n // 2 - size // 2
    return max(start, 0), min(start + size, n)


def workspace_layout(P, H, W, psf_patch, border_pixels, radii):
    """The sections of the workspace (include/kimg.h), in floats, of a [P][H][W] image with the
    patch ``psf_patch`` (P, h, w), a border in pixels and the scales' radii: the starts of ``coef``,
    ``taps``, ``tile_max``, ``tile_pos``, of ``res[k]`` (k >= 1) and of ``cross[j, k]`` (with its
    shape), ``tile_pitch`` and ``total``."""
    K = len(radii)
    r64 = lambda n: (n + 63) // 64 * 64     # noqa: E731
    tiles = (-(-(H - 2 * border_pixels) // TILE), -(-(W - 2 * border_pixels) // TILE))
    tile_pitch = r64(tiles[0] * tiles[1])
    image = r64(P * H * W)
    at = 64 + 64
    lay = dict(coef=64, taps=at, tile_pitch=tile_pitch)
    at += MAX_SCALES * _TAPS_PITCH + r64(MAX_SCALES * (MAX_SCALES + 1) // 2 * _CROSS_PITCH)
    lay['tile_max'] = at
    at += K * tile_pitch
    lay['tile_pos'] = at
    at += 2 * K * tile_pitch
    lay['res'] = {}
    for k in range(1, K):
        lay['res'][k] = at
        at += image
    lay['cross'] = {}
    for j in range(K):
        for k in range(K):
            R = radii[j] + radii[k]
            y0, y1 = crop_range(H, psf_patch[1], R)
            x0, x1 = crop_range(W, psf_patch[2], R)
            lay['cross'][j, k] = (at, (P, y1 - y0, x1 - x0))
            at += r64(P * (y1 - y0) * (x1 - x0))
    at += 2 * image
    lay['total'] = at
    return lay


# ---- the numpy twin -------------------------------------------------------------------------

def _conv_axis(a, taps):
    """One pass along the last axis: acc = 0, then acc = acc + t[i] * in[c - R + i] for i in order,
    taps outside the image skipped; float32 throughout."""
    R = (len(taps) - 1) // 2
    n = a.shape[-1]
    acc = np.zeros(a.shape, np.float32)
    for i in range(2 * R + 1):
        lo, hi = max(0, R - i), min(n, n + R - i)
        if lo < hi:
            acc[..., lo:hi] = acc[..., lo:hi] + np.float32(taps[i]) * a[..., lo - R + i:hi - R + i]
    return acc


def conv_host(image, taps):
    """conv(img, t): the horizontal pass into a temporary, then the vertical pass, of every plane."""
    image = np.asarray(image)
    types.require_float32(image.dtype, 'conv_host')
    taps = np.asarray(taps, np.float32)
    tmp = _conv_axis(image, taps)
    return np.ascontiguousarray(np.swapaxes(_conv_axis(np.swapaxes(tmp, -1, -2), taps), -1, -2))


class MultiScaleCleanHost:
    """The executable specification of the operator: exactly the arithmetic of include/kimg.h,
    "Multi-scale CLEAN", and nothing cleverer.  ``image`` (the dirty image, float32 [P][H][W]) and
    ``model`` are updated in place; ``image`` IS the residual of scale 0.  ``mask``: bool / uint8
    [H][W] or None."""

    def __init__(self, params, border, loop_gain, mode, image, psf, model, mask=None):
        if mode != CLEAN_I:
            raise ValueError('multi-scale CLEAN runs in mode CLEAN_I only')
        for a in (image, psf, model):
            types.require_float32(a.dtype, 'MultiScaleCleanHost')
        P, H, W = image.shape
        if psf.shape != image.shape or model.shape != image.shape:
            raise ValueError('image, psf and model must have one shape')
        if psf[0, H // 2, W // 2] != 1:
            raise ValueError('the centre of the PSF must be exactly 1')
        self.params = params
        self.loop_gain = np.float32(loop_gain)
        self.image, self.psf, self.model = image, psf, model
        self.mask = None if mask is None else np.asarray(mask) != 0
        self.border_pixels = border_pixels(border, image.shape, checked=False)
        bp = self.border_pixels
        K = len(params)
        self.tiles = (-(-(H - 2 * bp) // TILE), -(-(W - 2 * bp) // TILE))
        self.tile_max = np.zeros((K,) + self.tiles, np.float32)
        self.tile_pos = np.zeros((K,) + self.tiles + (2,), np.int32)
        self.residuals = [image] + [None] * (K - 1)
        self.norms = self.inv = None
        self.cross = {}
        self._patch = None
        self._stale = True

    # -- set-up
    def prepare(self, psf_patch):
        """What depends on the PSF and its patch (n_k, inv_k, the cross patches), then whatever a
        :meth:`reset` left to do."""
        if self._patch != tuple(psf_patch):
            P, H, W = self.image.shape
            K = len(self.params)
            ph, pw = psf_patch[1], psf_patch[2]
            full = {}
            self.norms = np.zeros(K, np.float32)
            for j in range(K):
                for k in range(j, K):
                    full[j, k] = conv_host(self.psf, self.params.cross_taps(j, k))
                self.norms[j] = full[j, j][0, H // 2, W // 2]
            self.inv = (np.float32(1.0) / self.norms).astype(np.float32)
            for j in range(K):
                for k in range(K):
                    R = self.params.radii[j] + self.params.radii[k]
                    y0, y1 = crop_range(H, ph, R)
                    x0, x1 = crop_range(W, pw, R)
                    self.cross[j, k] = full[min(j, k), max(j, k)][:, y0:y1, x0:x1] * self.inv[j]
            self._patch = tuple(psf_patch)
        if self._stale:
            for k in range(1, len(self.params)):
                self.residuals[k] = conv_host(self.image, self.params.taps[k]) * self.inv[k]
            self._update_tiles(0, 0, self.tiles[0], self.tiles[1])
            self._stale = False

    def reset(self):
        """The residuals of the scales k >= 1 and every tile are rebuilt from the image (and the
        mask) as they stand, before the next cycle."""
        self._stale = True

    def _update_tiles(self, ty0, tx0, ty1, tx1, scales=None):
        P, H, W = self.image.shape
        bp = self.border_pixels
        for k in range(len(self.params)) if scales is None else scales:
            plane = np.abs(self.residuals[k][0])
            for ty in range(ty0, ty1):
                for tx in range(tx0, tx1):
                    y0, x0 = ty * TILE + bp, tx * TILE + bp
                    y1, x1 = min(y0 + TILE, H - bp), min(x0 + TILE, W - bp)
                    tile = plane[y0:y1, x0:x1]
                    if self.mask is not None:
                        tile = np.where(self.mask[y0:y1, x0:x1], tile, np.float32(0))
                    at = int(np.argmax(tile))           # the first maximum in row-major order
                    value = tile.flat[at]
                    if value > 0:
                        self.tile_max[k, ty, tx] = value
                        self.tile_pos[k, ty, tx] = (y0 + at // (x1 - x0), x0 + at % (x1 - x0))
                    else:       # the host scan's start position, (x0, y0) in the (y, x) slots
                        self.tile_max[k, ty, tx] = 0
                        self.tile_pos[k, ty, tx] = (x0, y0)

    # -- cycles
    def _cycle(self, psf_patch, threshold):
        P, H, W = self.image.shape
        K = len(self.params)
        ph, pw = psf_patch[1], psf_patch[2]
        best = None
        for k in range(K):
            tile = int(np.argmax(self.tile_max[k]))     # the first maximal tile
            peak = self.tile_max[k].flat[tile]
            biased = self.params.biases[k] * peak       # float32
            if best is None or biased > best[0]:
                best = (biased, k, tile, peak)
        _, ks, tile, peak = best
        if peak < np.float32(threshold) or (self.mask is not None and peak == 0):
            return None
        y, x = (int(v) for v in self.tile_pos[ks].reshape(-1, 2)[tile])
        a = (self.loop_gain * self.residuals[ks][:, y, x]).astype(np.float32)
        bp = self.border_pixels
        for j in range(K):
            R = self.params.radii[j] + self.params.radii[ks]
            bh, bw = ph + 2 * R, pw + 2 * R
            by0, bx0 = y - bh // 2, x - bw // 2
            cy0, cy1 = crop_range(H, ph, R)
            cx0, cx1 = crop_range(W, pw, R)
            # the box clipped to the image and to what the cross patch holds (q = centre + offset)
            y0 = max(0, by0, y - H // 2 + cy0)
            y1 = min(H, by0 + bh, y - H // 2 + cy1)
            x0 = max(0, bx0, x - W // 2 + cx0)
            x1 = min(W, bx0 + bw, x - W // 2 + cx1)
            if y0 < y1 and x0 < x1:
                X = self.cross[j, ks][:, y0 - y + H // 2 - cy0:y1 - y + H // 2 - cy0,
                                      x0 - x + W // 2 - cx0:x1 - x + W // 2 - cx0]
                self.residuals[j][:, y0:y1, x0:x1] = \
                    self.residuals[j][:, y0:y1, x0:x1] - a[:, np.newaxis, np.newaxis] * X
            ty0 = max((max(by0, 0) - bp) // TILE, 0)
            tx0 = max((max(bx0, 0) - bp) // TILE, 0)
            ty1 = min(-(-(min(by0 + bh, H) - bp) // TILE), self.tiles[0])
            tx1 = min(-(-(min(bx0 + bw, W) - bp) // TILE), self.tiles[1])
            self._update_tiles(ty0, tx0, ty1, tx1, scales=[j])
        t = self.params.taps[ks]
        R = self.params.radii[ks]
        weight = t[:, np.newaxis] * t[np.newaxis, :]           # float32, rounded first
        y0, y1 = max(0, y - R), min(H, y + R + 1)
        x0, x1 = max(0, x - R), min(W, x + R + 1)
        w = weight[y0 - y + R:y1 - y + R, x0 - x + R:x1 - x + R]
        self.model[:, y0:y1, x0:x1] = self.model[:, y0:y1, x0:x1] + a[:, np.newaxis, np.newaxis] * w
        return ks, y, x, peak, a

    def run_cycles(self, psf_patch, threshold, max_cycles):
        """Up to ``max_cycles`` cycles; the log as a structured array (:func:`log_dtype`)."""
        self.prepare(psf_patch)
        log = np.zeros(max(max_cycles, 0), log_dtype(self.image.shape[0]))
        for i in range(max_cycles):
            got = self._cycle(psf_patch, threshold)
            if got is None:
                return log[:i]
            log[i] = got
        return log


# ---- the device operator --------------------------------------------------------------------

class MultiScaleClean(accel.Operation):
    """Multi-scale minor cycles on the device.  Slots: **dirty** (the residual of scale 0),
    **model**, **psf** (all [P][H][W]) and the optional **mask** (uint8 [H][W], as for
    :class:`clean.Clean`).  Everything else lives in one workspace that is allocated at the first
    :meth:`prepare`.  Call :meth:`reset` once the buffers are populated (``new_psf=False`` where
    only the dirty image has changed since the last one), then :meth:`run_cycles`."""

    def __init__(self, template, command_queue, image_parameters, allocator=None):
        if image_parameters.fixed.real_dtype != template.dtype:
            raise ValueError('dtype mismatch')
        super().__init__(command_queue, allocator)
        self.template = template
        shape = (len(image_parameters.fixed.polarizations),
                 image_parameters.pixels, image_parameters.pixels)
        check_polarizations(template, shape)
        self.border_pixels = border_pixels(template.clean_parameters.border, shape)
        self.tiles = (accel.divup(shape[1] - 2 * self.border_pixels, TILE),
                      accel.divup(shape[2] - 2 * self.border_pixels, TILE))
        self.slots['dirty'] = accel.IOSlot(shape, template.dtype)
        self.slots['model'] = accel.IOSlot(shape, template.dtype)
        self.slots['psf'] = accel.IOSlot(shape, template.dtype)
        self.slots['mask'] = accel.IOSlot(shape[1:], np.uint8, optional=True)
        params = template.multiscale_parameters
        K = len(params)
        self._radii = (ctypes.c_int * K)(*params.radii)
        self._biases = (ctypes.c_float * K)(*[float(b) for b in params.biases])
        taps = np.zeros((K, _TAPS_PITCH), np.float32)
        for k, t in enumerate(params.taps):
            taps[k, :len(t)] = t
        pairs = [(j, k) for j in range(K) for k in range(j, K)]
        cross = np.zeros((len(pairs), _CROSS_PITCH), np.float32)
        for i, pair in enumerate(pairs):
            cross[i, :len(params.cross[pair])] = params.cross[pair]
        self._taps, self._cross_taps = taps, cross
        self._workspace = None
        self._layout = None
        self._patch = None
        self._pending = _SETUP_PSF | _SETUP_RESIDUALS
        self._log = None
        self.cycles_done = 0

    def ensure_all_bound(self):
        for name, slot in self.slots.items():
            if name != 'mask':
                self.ensure_bound(name)

    def _run(self):
        raise NotImplementedError('use reset() and run_cycles()')

    def _make_layout(self, psf_patch):
        P, H, W = self.buffer('dirty').shape
        return workspace_layout(P, H, W, psf_patch, self.border_pixels, self._radii)

    def reset(self, new_psf=True):
        """The residuals of the scales k >= 1 and every tile record are rebuilt from the dirty
        image (and the mask) as they stand -- with ``new_psf`` also n_k and the cross patches from
        the PSF -- before the next cycle (enqueued by :meth:`prepare`, which needs the patch)."""
        self._pending |= _SETUP_RESIDUALS | (_SETUP_PSF if new_psf else 0)

    def _mask_args(self):
        mask = self.buffer('mask')
        if mask is None:
            return None, 0
        mask.used_on(self.command_queue)
        return mask.ptr, mask.shape[1]

    def prepare(self, psf_patch):
        """Enqueue whatever set-up is pending for this patch."""
        self.ensure_all_bound()
        patch = tuple(int(x) for x in psf_patch)
        P, H, W = self.buffer('dirty').shape
        if patch != self._patch:
            self._pending |= _SETUP_PSF | _SETUP_RESIDUALS
            nbytes = lib().kimg_clean_scales_workspace_bytes(
                W, H, P, patch[2], patch[1], self.border_pixels, len(self._radii), self._radii)
            if nbytes == 0:
                raise ValueError('bad multi-scale CLEAN geometry')
            layout = self._make_layout(patch)
            assert layout['total'] * 4 == nbytes, 'workspace layout out of step with libkimg'
            if self._workspace is None or self._workspace.shape[0] * 4 < nbytes:
                self._workspace = accel.DeviceArray(self.command_queue.context, (nbytes // 4,),
                                                    np.float32, queue=self.command_queue)
            self._layout = layout
            self._patch = patch
        if not self._pending:
            return
        dirty, psf = self.buffer('dirty'), self.buffer('psf')
        mask_ptr, mask_row = self._mask_args()
        rc = lib().kimg_clean_scales_setup(
            dirty.ptr, *plane_pitches(dirty), *plane_args(psf), patch[2], patch[1],
            self.border_pixels, len(self._radii), self._radii,
            self._taps.ctypes.data, self._cross_taps.ctypes.data, self._pending,
            mask_ptr, mask_row, self._workspace.ptr, self._workspace.shape[0] * 4,
            self.command_queue.handle)
        if rc == -10001 and self._pending & _SETUP_PSF:
            centre = np.zeros(1, np.float32)
            psf.get_region(self.command_queue, centre, np.s_[0, H // 2, W // 2], np.s_[0])
            if centre[0] != 1:
                raise ValueError('the centre of the PSF must be exactly 1, not {!r}'.format(centre[0]))
        check(rc, 'kimg_clean_scales_setup')
        self._pending = 0

    def run_cycles(self, psf_patch, threshold, max_cycles):
        """Up to ``max_cycles`` cycles on the device, the host looking at the device once per 64
        of them; the log (:func:`log_dtype`) is read back once."""
        self.prepare(psf_patch)
        P, H, W = self.buffer('dirty').shape
        self.cycles_done = 0
        if max_cycles <= 0:
            return np.zeros(0, log_dtype(P))
        if self._log is None or self._log.shape[0] < max_cycles:
            self._log = accel.DeviceArray(self.command_queue.context, (max_cycles, 4 + P),
                                          np.float32, queue=self.command_queue)
        cp = self.template.clean_parameters
        dirty, model = self.buffer('dirty'), self.buffer('model')
        mask_ptr, mask_row = self._mask_args()
        done = ctypes.c_int(0)
        rc = lib().kimg_clean_scales_cycles(
            dirty.ptr, model.ptr, *plane_args(dirty)[1:], self._patch[2], self._patch[1],
            self.border_pixels, cp.mode, cp.loop_gain, threshold, len(self._radii), self._radii,
            self._biases, max_cycles, mask_ptr, mask_row, self._workspace.ptr,
            self._workspace.shape[0] * 4, self._log.ptr, ctypes.byref(done),
            self.command_queue.handle)
        check(rc, 'kimg_clean_scales_cycles')
        self.cycles_done = int(done.value)
        out = np.zeros(self.cycles_done, log_dtype(P))
        if self.cycles_done:
            rows = np.empty((self.cycles_done, 4 + P), np.float32)
            self._log.get_region(self.command_queue, rows, np.s_[:self.cycles_done], np.s_[:])
            ints = rows[:, :3].copy().view(np.int32)
            out['scale'], out['y'], out['x'] = ints[:, 0], ints[:, 1], ints[:, 2]
            out['peak'] = rows[:, 3]
            out['flux'] = rows[:, 4:]
        return out

    # -- what the set-up and the cycles keep on the device, for tests and tools
    def _section(self, start, count):
        host = np.empty(count, np.float32)
        self._workspace.get_region(self.command_queue, host, np.s_[start:start + count], np.s_[:])
        return host

    def scale_norms(self):
        """(n_k, inv_k), float32 [K] each."""
        coef = self._section(self._layout['coef'], 16)
        K = len(self._radii)
        return coef[:K].copy(), coef[8:8 + K].copy()

    def residual(self, k):
        if k == 0:
            return self.buffer('dirty').get(self.command_queue)
        P, H, W = self.buffer('dirty').shape
        return self._section(self._layout['res'][k], P * H * W).reshape(P, H, W)

    def cross_patch(self, j, k):
        start, shape = self._layout['cross'][j, k]
        return self._section(start, int(np.prod(shape))).reshape(shape)

    def tile_records(self):
        """(tile_max float32 [K][ty][tx], tile_pos int32 [K][ty][tx][2])."""
        K, lay = len(self._radii), self._layout
        n = self.tiles[0] * self.tiles[1]
        tmax = self._section(lay['tile_max'], K * lay['tile_pitch']).reshape(K, -1)[:, :n]
        tpos = self._section(lay['tile_pos'], 2 * K * lay['tile_pitch']).view(np.int32)
        tpos = tpos.reshape(K, -1)[:, :2 * n]
        return tmax.reshape((K,) + self.tiles).copy(), tpos.reshape((K,) + self.tiles + (2,)).copy()


class MultiScaleCleanTemplate(ImageTemplate):
    """The constructor shape of :class:`clean.CleanTemplate` plus the scales."""
    operator = MultiScaleClean

    def __init__(self, context, clean_parameters, multiscale_parameters, dtype, num_polarizations,
                 tuning=None):
        super().__init__(context, dtype, num_polarizations, tuning)
        if clean_parameters.mode != CLEAN_I:
            raise ValueError('multi-scale CLEAN runs in mode CLEAN_I only')
        self.clean_parameters = clean_parameters
        self.multiscale_parameters = multiscale_parameters


def convolve_separable(command_queue, src, dest, taps, tmp=None):
    """``dest = conv(src, taps)`` on device arrays [P][H][W] (kimg_image_convolve_separable);
    ``taps``: host float32 [2 R + 1]."""
    types.require_float32(src.dtype, 'convolve_separable')
    taps = np.ascontiguousarray(taps, np.float32)
    R = (len(taps) - 1) // 2
    if len(taps) != 2 * R + 1:
        raise ValueError('an odd number of taps')
    if R > MAX_RADIUS:
        raise ValueError('radius {} exceeds {}'.format(R, MAX_RADIUS))
    ctx = command_queue.context
    if tmp is None:
        tmp = accel.DeviceArray(ctx, src.shape, np.float32, queue=command_queue)
    dtaps = accel.DeviceArray(ctx, taps.shape, np.float32, queue=command_queue)
    dtaps.set(command_queue, taps)
    rc = lib().kimg_image_convolve_separable(
        src.ptr, *plane_pitches(src), dest.ptr, *plane_pitches(src), tmp.ptr,
        *plane_args(src)[1:], dtaps.ptr, R,
        command_queue.handle)
    check(rc, 'kimg_image_convolve_separable')
