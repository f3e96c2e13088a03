"""What the two test modules of multi-scale CLEAN on non-square, padded and wide images share
(test_multiscale_cases_host.py, test_multiscale_abi_gpu.py): the field generator, the cases, the
buffer layouts a C caller may hand over, a restatement of which form of the residual update a
thread takes, and the operator driven through the C ABI on such buffers."""
import ctypes

import numpy as np

from helpers import Padded

from katsdpimager_amd import multiscale as ms
from katsdpimager_amd.image_plane import border_pixels
from katsdpimager_amd.parameters import CLEAN_I

TILE = 32
LOOP_GAIN = 0.1
SETUP_PSF, SETUP_RESIDUALS = 1, 2          # KIMG_CLEAN_SCALES_PSF, _RESIDUALS
GUARD = 256                                 # floats of sentinel after the workspace
GUARD_VALUE = np.float32(-2.5e38)


# ---- the field ----------------------------------------------------------------------------------

def edge_spots(H, W, bp):
    """Blobs and points 3 pixels inside the border on each of the four sides and in the corners,
    and two in the interior: (y, x, FWHM, amplitude)."""
    ylo, yhi, xlo, xhi = bp + 3, H - bp - 4, bp + 3, W - bp - 4
    cy, cx = H // 2, W // 2
    return [(ylo, xlo, 6, 6.0), (ylo, xhi, 0, -4.0), (yhi, xlo, 3, 5.0), (yhi, xhi, 8, -7.0),
            (cy, xlo, 0, 3.0), (min(cy + 5, yhi), max(cx - 9, xlo), 9, 8.0), (yhi, cx, 4, 4.0),
            (ylo, cx + 7, 5, -5.5), (cy - 2, xhi, 7, 6.5)]


def field(H, W, P, border_pixels, seed, spots, noise=0.05):
    """(dirty, psf), float32 [P][H][W]: noise plus the Gaussian blobs and points ``spots`` ((y, x,
    FWHM, amplitude), FWHM 0 = one pixel wide), polarization p scaled by 1 - 0.3 p; a Gaussian-core
    PSF with noisy wings whose centre [H // 2, W // 2] is exactly 1.  ``spots=None``:
    :func:`edge_spots` of the border."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W].astype(np.float64)
    cy, cx = H // 2, W // 2
    psf = np.empty((P, H, W), np.float32)
    for p in range(P):
        psf[p] = np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * 1.7 ** 2)) \
            + 0.01 * rng.standard_normal((H, W))
    psf /= psf[:, cy, cx][:, None, None]
    assert np.all(psf[:, cy, cx] == 1)
    dirty = noise * rng.standard_normal((P, H, W))
    if spots is None:
        spots = edge_spots(H, W, border_pixels)
    for (y, x, fwhm, amp) in spots:
        s = max(fwhm, 1.0) / 2.355
        blob = amp * np.exp(-((yy - y) ** 2 + (xx - x) ** 2) / (2 * s * s))
        for p in range(P):
            dirty[p] += blob * (1.0 - 0.3 * p)
    return dirty.astype(np.float32), psf


# ---- the cases ----------------------------------------------------------------------------------

class Case:
    def __init__(self, name, shape, P, bp, scales, patch, cycles, seed, spots=None, biases=None,
                 noise=0.05):
        self.name, self.P, self.bp, self.scales = name, P, bp, scales
        self.H, self.W = shape
        self.patch = (P,) + tuple(patch)            # (P, h, w), as the operators take it
        self.cycles, self.seed, self.spots, self.biases, self.noise = cycles, seed, spots, biases, noise
        self.params = ms.MultiScaleParameters(scales, biases)
        self.K = len(self.params)
        # the twin takes a fraction of the smaller side
        self.border = bp / min(shape)
        assert border_pixels(self.border, (P,) + tuple(shape), checked=False) == bp
        self.tiles = (-(-(self.H - 2 * bp) // TILE), -(-(self.W - 2 * bp) // TILE))
        self._field = self._reference = None

    def field(self):
        """(dirty, psf), made once; callers copy what they change."""
        if self._field is None:
            self._field = field(self.H, self.W, self.P, self.bp, self.seed, self.spots, self.noise)
            for a in self._field:
                a.setflags(write=False)
        return self._field

    def twin(self, dirty=None, psf=None, model=None, mask=None):
        d, f = self.field()
        dirty = d.copy() if dirty is None else dirty
        model = np.zeros_like(dirty) if model is None else model
        return ms.MultiScaleCleanHost(self.params, self.border, LOOP_GAIN, CLEAN_I, dirty,
                                      f if psf is None else psf, model, mask=mask)

    def reference(self):
        """The twin after ``cycles`` cycles at threshold 0 without a mask, its state after the set-up
        alone, and its log; computed once and left as it is."""
        if self._reference is None:
            twin = self.twin()
            twin.prepare(self.patch)
            setup = dict(residuals=[r.copy() for r in twin.residuals],
                         tile_max=twin.tile_max.copy(), tile_pos=twin.tile_pos.copy())
            log = twin.run_cycles(self.patch, 0.0, self.cycles)
            self._reference = (twin, setup, log)
        return self._reference

    def layout(self):
        """The workspace sections, in floats."""
        return ms.workspace_layout(self.P, self.H, self.W, self.patch, self.bp, self.params.radii)


_MANY = (544, 2016)
CASES = {c.name: c for c in [
    Case('wide', (72, 300), 2, 4, [0, 4, 9], (15, 17), 120, 41),
    Case('tall', (300, 72), 1, 4, [0, 4, 9], (17, 15), 120, 42),
    # 98 = 2 mod 4 with an odd border: x is odd, y * 98 even, 71 * 98 = 2 mod 4 -- no thread of any
    # plane of any scale sits on a 16-byte boundary at compact pitch; 65 x 92 interior: partial
    # tiles both ways
    Case('odd', (71, 98), 3, 3, [0, 4, 9], (15, 17), 120, 43),
    # an odd width: at compact pitch every fourth row is aligned, in the workspace's residuals of
    # the scales k >= 1 as well, whose pitch no buffer layout changes
    Case('odd_width', (70, 99), 3, 3, [0, 4, 9], (15, 17), 120, 43),
    # one broad blob off the centre; equal biases, so that the smoothed residual wins at first
    Case('tiny', (5, 7), 1, 0, [0, 1.5], (3, 3), 20, 44, spots=[(2, 4, 3, 2.0), (4, 0, 0, -1.5)],
         biases=[1.0, 1.0]),
    # the brightest source in the last tile (16, 62) = 1070; the others in tiles below 1024
    Case('many_tiles', _MANY, 1, 0, [0, 4], (15, 17), 40, 45,
         spots=[(530, 2000, 5, 9.0), (520, 1990, 0, 5.0), (3, 3, 4, 6.0), (300, 1000, 6, -7.0),
                (540, 40, 0, 4.0), (10, 2010, 3, -5.0), (535, 1500, 4, 6.5)]),
    # points, narrow blobs and two broad ones beside the edge spots: every one of the six is taken
    Case('six', (96, 272), 1, 4, [0, 4, 9, 18, 30, 50], (15, 17), 100, 46,
         spots=edge_spots(96, 272, 4) + [(30, 60, 0, 25.0), (70, 200, 0, -20.0), (48, 200, 30, 3.0),
                                         (45, 80, 50, -3.0), (20, 150, 4, 30.0), (75, 120, 4, -28.0)]),
]}

# ---- the buffer layouts -------------------------------------------------------------------------
LAYOUTS = ('compact', 'pitch+1', 'pitch+4', 'offset')


def padding(layout, W):
    """Padded's (rpad, vpad, origin) of the dirty image and the model, and of the PSF -- which has
    pitches of its own in every layout but ``compact``."""
    if layout == 'compact':
        return dict(rpad=0, vpad=0, origin=(0, 0)), dict(rpad=0, vpad=0, origin=(0, 0))
    if layout == 'pitch+1':             # row pitch = 1 mod 4: every fourth row is 16-byte aligned
        rpad = next(r for r in range(1, 5) if (W + r) % 4 == 1)
        return dict(rpad=rpad, vpad=0, origin=(0, 0)), dict(rpad=rpad + 2, vpad=1, origin=(0, 0))
    if layout == 'pitch+4':
        return dict(rpad=4, vpad=2, origin=(0, 0)), dict(rpad=7, vpad=0, origin=(1, 0))
    if layout == 'offset':
        return dict(rpad=5, vpad=1, origin=(2, 3)), dict(rpad=2, vpad=3, origin=(1, 6))
    raise KeyError(layout)


MASK_PADDING = dict(rpad=3, vpad=2, origin=(1, 2))         # mask_row_pitch = W + 5


def pitches(case, layout):
    """(offset of the interior from the 16-byte aligned base, row pitch, polarization pitch) of the
    dirty image under ``layout``, in floats: what Padded makes of :func:`padding`."""
    pad = padding(layout, case.W)[0]
    oy, ox = pad['origin']
    row = ox + case.W + pad['rpad']
    return oy * row + ox, row, (oy + case.H + pad['vpad']) * row


# ---- which form of the update a thread takes ----------------------------------------------------

def update_forms(case, layout, log):
    """For every cycle of ``log``, scale j, polarization p and lattice block that the box of scale j
    touches: ``(cycle, j, p, ly, lx, ys, vec, lanes)``.  ``ys`` are the block's rows inside the
    image, ``vec`` [rows][8] says whether the thread that owns the pixels x4 .. x4 + 3 of that row
    sits on a 16-byte aligned address with all four inside the row (the device then takes one
    16-byte load and store, else four scalar ones), ``lanes`` [rows][8] how many of its four pixels
    the cycle changes.  Geometry only: the residual of scale 0 lives in the caller's buffer with its
    offset and pitches, the residuals of the scales k >= 1 in the 16-byte aligned workspace at the
    pitch of the image's width."""
    H, W, P, bp = case.H, case.W, case.P, case.bp
    lay = case.layout()
    radii = case.params.radii
    ph, pw = case.patch[1], case.patch[2]
    for cycle, entry in enumerate(log):
        ks, y, x = int(entry['scale']), int(entry['y']), int(entry['x'])
        for j in range(case.K):
            if j == 0:
                offset, row, pol = pitches(case, layout)
            else:
                offset, row, pol = lay['res'][j], W, H * W
            R = radii[j] + radii[ks]
            bh, bw = ph + 2 * R, pw + 2 * R
            by0, bx0 = y - bh // 2, x - bw // 2
            cy0, cy1 = ms.crop_range(H, ph, R)
            cx0, cx1 = ms.crop_range(W, pw, R)
            # the pixels the cycle changes: the box within the image and within what X holds
            y0, y1 = max(0, by0, y - H // 2 + cy0), min(H, by0 + bh, y - H // 2 + cy1)
            x0, x1 = max(0, bx0, x - W // 2 + cx0), min(W, bx0 + bw, x - W // 2 + cx1)
            for ly in range((by0 - bp) // TILE, (by0 + bh - 1 - bp) // TILE + 1):
                Y0 = bp + ly * TILE
                ys = np.arange(max(Y0, 0), min(Y0 + TILE, H))
                if len(ys) == 0:
                    continue
                for lx in range((bx0 - bp) // TILE, (bx0 + bw - 1 - bp) // TILE + 1):
                    X0 = bp + lx * TILE
                    if X0 + TILE <= 0 or X0 >= W:
                        continue
                    x4 = X0 + 4 * np.arange(8)
                    xs = x4[:, None] + np.arange(4)[None, :]                    # [8][4]
                    in_x = ((xs >= x0) & (xs < x1)).sum(axis=1)                 # [8]
                    in_y = (ys >= y0) & (ys < y1)                               # [rows]
                    lanes = in_y[:, None] * in_x[None, :]
                    inside = (x4 >= 0) & (x4 + 3 < W)
                    for p in range(P):
                        address = (offset + p * pol + ys[:, None] * row + x4[None, :]) * 4
                        vec = (address % 16 == 0) & inside[None, :]
                        yield cycle, j, p, ly, lx, ys, vec, lanes


def forms_taken(case, layout, log):
    """A summary of :func:`update_forms`: for every (j, p) the number of threads that change pixels
    through the 16-byte form (``vec``), through it with only some of their four pixels changed
    (``partial``: the store that is gated on any lane having changed, at a box edge) and through
    the scalar form (``scalar``); and ``mixed``, the number of blocks in which both forms change
    pixels."""
    out = {(j, p): dict(vec=0, partial=0, scalar=0, mixed=0)
           for j in range(case.K) for p in range(case.P)}
    for cycle, j, p, ly, lx, ys, vec, lanes in update_forms(case, layout, log):
        work = lanes > 0
        n_vec, n_scalar = int((vec & work).sum()), int((~vec & work).sum())
        c = out[j, p]
        c['vec'] += n_vec
        c['partial'] += int((vec & work & (lanes < 4)).sum())
        c['scalar'] += n_scalar
        c['mixed'] += int(n_vec > 0 and n_scalar > 0)
    return out


# ---- the operator through the C ABI -------------------------------------------------------------

def blocky_mask(case, seed=5):
    """A blocky random mask plus one full column."""
    rng = np.random.default_rng(seed)
    H, W = case.H, case.W
    mask = np.kron(rng.random((-(-H // 8), -(-W // 8))) < 0.4, np.ones((8, 8), bool))[:H, :W].copy()
    mask[:, W // 2 + 3] = True
    return mask


class Bound:
    """The buffers of one case under one layout on the device, and the calls on them."""

    def __init__(self, ctx, q, case, layout, dirty=None, psf=None, mask=None):
        from katsdpimager_amd import accel
        from katsdpimager_amd._lib import lib
        self.ctx, self.q, self.case, self.layout_name = ctx, q, case, layout
        d, f = case.field()
        self.dirty0 = d if dirty is None else dirty
        self.psf0 = f if psf is None else psf
        self.mask0 = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        pad, psf_pad = padding(layout, case.W)
        self.dirty = Padded(ctx, q, self.dirty0, **pad)
        self.model = Padded(ctx, q, np.zeros_like(self.dirty0), **pad)
        self.psf = Padded(ctx, q, self.psf0, **psf_pad)
        self.mask = None if mask is None else Padded(ctx, q, self.mask0, **MASK_PADDING)
        for buf in (self.dirty, self.model, self.psf):
            assert buf.dev.ptr % 16 == 0
        assert (self.dirty.offset, self.dirty.row, self.dirty.pol) == pitches(case, layout)
        assert (self.model.row, self.model.pol) == (self.dirty.row, self.dirty.pol)
        if layout != 'compact':
            assert (self.psf.row, self.psf.pol) != (self.dirty.row, self.dirty.pol)
        if self.mask is not None:
            assert self.mask.row == case.W + 5
        K = case.K
        self.radii = (ctypes.c_int * K)(*case.params.radii)
        self.biases = (ctypes.c_float * K)(*[float(b) for b in case.params.biases])
        self.nbytes = lib().kimg_clean_scales_workspace_bytes(
            case.W, case.H, case.P, case.patch[2], case.patch[1], case.bp, K, self.radii)
        self.lay = case.layout()
        assert self.nbytes == 4 * self.lay['total'] > 0
        self.workspace = accel.DeviceArray(ctx, (self.nbytes // 4 + GUARD,), np.float32, queue=q)
        assert self.workspace.ptr % 16 == 0
        self.workspace.set(q, np.full(self.nbytes // 4 + GUARD, GUARD_VALUE, np.float32))
        taps = np.zeros((K, 192), np.float32)
        for k, t in enumerate(case.params.taps):
            taps[k, :len(t)] = t
        pairs = [(j, k) for j in range(K) for k in range(j, K)]
        cross = np.zeros((len(pairs), 320), np.float32)
        for i, pair in enumerate(pairs):
            cross[i, :len(case.params.cross[pair])] = case.params.cross[pair]
        self.taps, self.cross_taps = taps, cross
        self.log = None
        self.cycles_done = 0

    def _mask_args(self):
        return (None, 0) if self.mask is None else (self.mask.ptr, self.mask.row)

    def setup(self, what=SETUP_PSF | SETUP_RESIDUALS):
        from katsdpimager_amd._lib import lib, check
        c = self.case
        check(lib().kimg_clean_scales_setup(
            self.dirty.ptr, self.dirty.row, self.dirty.pol, self.psf.ptr, self.psf.row, self.psf.pol,
            c.W, c.H, c.P, c.patch[2], c.patch[1], c.bp, c.K, self.radii, self.taps.ctypes.data,
            self.cross_taps.ctypes.data, what, *self._mask_args(), self.workspace.ptr, self.nbytes,
            self.q.handle), 'kimg_clean_scales_setup')

    def cycles(self, threshold, max_cycles):
        """The log (ms.log_dtype) of up to ``max_cycles`` cycles; the log buffer has a guard of
        its own."""
        from katsdpimager_amd import accel
        from katsdpimager_amd._lib import lib, check
        c = self.case
        width = 4 + c.P
        dlog = accel.DeviceArray(self.ctx, (max_cycles * width + GUARD,), np.float32, queue=self.q)
        dlog.set(self.q, np.full(max_cycles * width + GUARD, GUARD_VALUE, np.float32))
        done = ctypes.c_int(-1)
        check(lib().kimg_clean_scales_cycles(
            self.dirty.ptr, self.model.ptr, self.dirty.row, self.dirty.pol, c.W, c.H, c.P,
            c.patch[2], c.patch[1], c.bp, CLEAN_I, LOOP_GAIN, threshold, c.K, self.radii,
            self.biases, max_cycles, *self._mask_args(), self.workspace.ptr, self.nbytes, dlog.ptr,
            ctypes.byref(done), self.q.handle), 'kimg_clean_scales_cycles')
        self.cycles_done = n = int(done.value)
        assert 0 <= n <= max_cycles
        rows = dlog.get(self.q)
        assert np.all(rows[n * width:].view(np.uint32) == GUARD_VALUE.view(np.uint32)), \
            'the log was written past its last entry'
        rows = rows[:n * width].reshape(n, width)
        out = np.zeros(n, ms.log_dtype(c.P))
        ints = rows[:, :3].copy().view(np.int32)
        out['scale'], out['y'], out['x'] = ints[:, 0], ints[:, 1], ints[:, 2]
        out['peak'] = rows[:, 3]
        out['flux'] = rows[:, 4:]
        return out

    # -- what the device holds
    def read_workspace(self):
        """The whole workspace, the guard checked."""
        ws = self.workspace.get(self.q)
        assert np.all(ws[self.nbytes // 4:].view(np.uint32) == GUARD_VALUE.view(np.uint32)), \
            'the guard after the workspace changed'
        return ws[:self.nbytes // 4]

    def norms(self, ws):
        coef = ws[self.lay['coef']:self.lay['coef'] + 16]
        return coef[:self.case.K].copy(), coef[8:8 + self.case.K].copy()

    def residual(self, ws, k):
        c = self.case
        if k == 0:
            return self.dirty.get(self.q)               # (checks the padding)
        start = self.lay['res'][k]
        return ws[start:start + c.P * c.H * c.W].reshape(c.P, c.H, c.W)

    def cross_patch(self, ws, j, k):
        start, shape = self.lay['cross'][j, k]
        return ws[start:start + int(np.prod(shape))].reshape(shape)

    def tile_records(self, ws):
        c, lay = self.case, self.lay
        n, pitch = c.tiles[0] * c.tiles[1], lay['tile_pitch']
        tmax = ws[lay['tile_max']:lay['tile_max'] + c.K * pitch].reshape(c.K, pitch)[:, :n]
        tpos = ws[lay['tile_pos']:lay['tile_pos'] + 2 * c.K * pitch].view(np.int32)
        tpos = tpos.reshape(c.K, 2 * pitch)[:, :2 * n]
        return tmax.reshape((c.K,) + c.tiles), tpos.reshape((c.K,) + c.tiles + (2,))

    def assert_inputs_untouched(self):
        """The PSF and the mask, interior and padding, are what they were."""
        np.testing.assert_array_equal(self.psf.get(self.q), self.psf0)
        if self.mask is not None:
            np.testing.assert_array_equal(self.mask.get(self.q), self.mask0)

    def assert_state(self, twin):
        """Residual of every scale, model and tile records equal the twin's; the padding of dirty
        and model, the PSF, the mask and the workspace guard are untouched."""
        ws = self.read_workspace()
        for k in range(self.case.K):
            np.testing.assert_array_equal(self.residual(ws, k), twin.residuals[k], 'residual %d' % k)
        np.testing.assert_array_equal(self.model.get(self.q), twin.model)
        tmax, tpos = self.tile_records(ws)
        np.testing.assert_array_equal(tmax, twin.tile_max)
        np.testing.assert_array_equal(tpos, twin.tile_pos)
        self.assert_inputs_untouched()
        return ws


def same_log(got, want):
    assert len(got) == len(want)
    for name in ('scale', 'y', 'x', 'peak', 'flux'):
        np.testing.assert_array_equal(got[name], want[name], name)
