"""CLEAN masks (clean windows): a per-pixel allow map for the minor cycle (include/kimg.h, "CLEAN
masks").  The reference has no mask, so the truth is a masked RESTATEMENT of its CleanHost in this
module: oracle.kimg_oracle.Clean with the tile scan replaced by a plain numpy scan that only admits
allowed pixels, and the stop at a best metric of exactly 0.  With an all-ones mask the restatement
is the pinned oracle bit for bit (CPU tests below); the HIP kernels are compared against it bit for
bit -- positions, metrics, model pixels, the final dirty and model images and the tile arrays -- in
the per-call, two-launch and one-launch forms (GPU tests)."""
import ctypes
import os
import re

import numpy as np
import pytest

import golden_inputs as gi
from oracle import kimg_oracle as orc
from test_clean_multi_model import sources_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu


# ---- the truth ---------------------------------------------------------------------------------
class MaskedClean(orc.Clean):
    """CleanHost restated with a mask: ``mask`` uint8/bool [H][W], one plane for all polarizations,
    nonzero = a component may be placed on the pixel.

    * a pixel is a candidate only inside the border and where allowed;
    * within a tile the first strict maximum in row-major order wins; a tile without a candidate of
      positive metric records 0 and the reference's (x0, y0) start position (clean.py:950);
    * subtraction is the reference's: the whole patch, masked pixels included;
    * a best metric of exactly 0 ends the search whatever the threshold."""

    def __init__(self, pixels, border, loop_gain, mode, image, psf, model, mask):
        super().__init__(pixels, border, loop_gain, mode, image, psf, model)
        self.mask = np.asarray(mask) != 0
        assert self.mask.shape == image.shape[1:]

    def _metric(self, y0, y1, x0, x1):
        region = self.image[:, y0:y1, x0:x1]
        if self.mode == 0:
            return np.abs(region[0])
        value = np.zeros(region.shape[1:], np.float32)
        for pol in range(region.shape[0]):          # (separately rounded, in polarization order)
            value = value + region[pol] * region[pol]
        return value

    def _update_tiles(self, ty0, tx0, ty1, tx1):
        H, W = self.image.shape[1:]
        ts, bp = self.tile_size, self.border_pixels
        for ty in range(ty0, ty1):
            for tx in range(tx0, tx1):
                x0, y0 = tx * ts + bp, ty * ts + bp
                x1, y1 = min(x0 + ts, W - bp), min(y0 + ts, H - bp)
                value = np.where(self.mask[y0:y1, x0:x1], self._metric(y0, y1, x0, x1), np.float32(0))
                best, best_pos = np.float32(0), (x0, y0)        # clean.py:950
                if value.size and np.nanmax(value) > 0:
                    flat = int(np.nanargmax(value))     # first occurrence = first strict maximum
                    best = value.flat[flat]
                    best_pos = (y0 + flat // (x1 - x0), x0 + flat % (x1 - x0))
                self._tile_max[ty, tx] = best
                self._tile_pos[ty, tx] = best_pos

    def __call__(self, psf_patch_, threshold=0.0):
        if np.max(self._tile_max) == 0:
            return None, None, None
        return super().__call__(psf_patch_, threshold)


def masked_run(G, border, loop_gain, mode, dirty, psf, patch, threshold, cycles, mask, ref=None):
    """As test_clean_multi_model.reference_run, on the restatement."""
    if ref is None:
        img, model = dirty.copy(), np.zeros_like(dirty)
        ref = MaskedClean(G, border, loop_gain, mode, img, psf, model, mask)
        ref.reset()
    log = []
    for _ in range(cycles):
        v, pos, pix = ref(patch, threshold)
        if v is None:
            break
        log.append((v, ref.last_pos, np.array(pix)))
    return log, ref.image, ref.model, ref._tile_max, ref._tile_pos


def plain_run(G, border, loop_gain, mode, dirty, psf, patch, threshold, cycles):
    img, model = dirty.copy(), np.zeros_like(dirty)
    ref = orc.Clean(G, border, loop_gain, mode, img, psf, model)
    ref.reset()
    log = []
    for _ in range(cycles):
        v, pos, pix = ref(patch, threshold)
        if v is None:
            break
        log.append((v, ref.last_pos, np.array(pix)))
    return log, img, model, ref._tile_max, ref._tile_pos


def same_run(got, want):
    assert len(got[0]) == len(want[0])
    for a, b in zip(got[0], want[0]):
        assert a[0] == b[0] and tuple(a[1]) == tuple(b[1]), (a, b)
        np.testing.assert_array_equal(a[2], b[2])
    for a, b in zip(got[1:], want[1:]):
        np.testing.assert_array_equal(a, b)


# ---- CPU: the restatement against the pinned oracle ----------------------------------------------
@pytest.mark.parametrize('name', list(gi.CLEAN_CONFIGS))
def test_all_ones_restatement_is_the_oracle_on_g7(golden, name):
    """The G7 problems: with every pixel allowed the restatement gives the component list, images
    and tile arrays of orc.Clean -- and with them the G7 golden's final images."""
    c = gi.CLEAN_CONFIGS[name]
    ci = gi.clean_inputs(c)
    args = (c['pixels'], c['border'], c['loop_gain'], c['mode'], ci['dirty'], ci['psf'],
            ci['psf_patch'], c['threshold'], c['cycles'])
    want = plain_run(*args)
    got = masked_run(*args, np.ones(ci['dirty'].shape[1:], np.uint8))
    same_run(got, want)
    g = golden('g7_clean_' + name)
    np.testing.assert_array_equal(got[1], g['dirty_final'])
    np.testing.assert_array_equal(got[2], g['model_final'])
    np.testing.assert_array_equal(np.array([a[1] for a in got[0]], np.int32).reshape(-1, 2), g['true_pos'])


@pytest.mark.parametrize('mode,P', [(0, 1), (1, 1), (0, 4), (1, 4)])
def test_all_ones_restatement_is_the_oracle(mode, P):
    """The G7 recipe with both metrics and 1 and 4 polarizations."""
    c = dict(gi.CLEAN_CONFIGS['i'], P=P, mode=mode, pixels=160, psf_patch=(P, 47, 33), cycles=120)
    ci = gi.clean_inputs(c)
    args = (c['pixels'], c['border'], c['loop_gain'], mode, ci['dirty'], ci['psf'], ci['psf_patch'],
            0.0, c['cycles'])
    same_run(masked_run(*args, np.ones((160, 160), bool)), plain_run(*args))


def test_restatement_semantics():
    """What the mask means, on a case small enough to see: candidates, empty tiles, the metric-0
    stop, and the subtraction reaching masked pixels."""
    G = 96
    psf = np.zeros((1, G, G), np.float32)
    psf[0, G // 2 - 2:G // 2 + 3, G // 2 - 2:G // 2 + 3] = 0.5
    psf[0, G // 2, G // 2] = 1.0
    dirty = np.zeros((1, G, G), np.float32)
    dirty[0, 10, 10] = 5.0          # brightest, masked
    dirty[0, 11, 11] = 2.0          # allowed, inside the patch of (10, 10)
    dirty[0, 70, 70] = 3.0          # allowed
    mask = np.zeros((G, G), np.uint8)
    mask[11, 11] = mask[70, 70] = 1
    log, img, model, tile_max, tile_pos = masked_run(G, 0.0, 0.5, 0, dirty, psf, (1, 5, 5), 0.0, 100, mask)
    assert [a[1] for a in log[:2]] == [(70, 70), (11, 11)]
    assert all(mask[a[1]] for a in log)
    assert img[0, 10, 10] != 5.0                # (subtraction around (11, 11) reached the masked pixel)
    assert set(zip(*np.nonzero(model[0]))) == {(11, 11), (70, 70)}
    assert tile_max[1, 1] == 0 and tuple(tile_pos[1, 1]) == (32, 32)       # an empty tile
    # all-masked: nothing at threshold 0
    log = masked_run(G, 0.0, 0.5, 0, dirty, psf, (1, 5, 5), 0.0, 10, np.zeros((G, G), np.uint8))[0]
    assert log == []


# ---- CPU: the ABI --------------------------------------------------------------------------------
MASKED_SYMBOLS = ('kimg_update_tiles_masked', 'kimg_find_peak_masked', 'kimg_clean_cycles_masked')


def test_masked_symbols_declared_exported_prototyped():
    from katsdpimager_amd import _lib, build
    build.build_lib()
    header = open(os.path.join(ROOT, 'include', 'kimg.h')).read()
    declared = set(re.findall(r'\b(kimg_[a-z0-9_]+)\s*\(', header))
    # (through _lib.lib(), which loads PyTorch's HIP runtime before the library: a process whose
    # first HIP runtime comes with a bare CDLL of the library finds no device later)
    handle = _lib.lib()
    for name in MASKED_SYMBOLS:
        assert name in declared, name
        assert hasattr(handle, name), name
        unmasked = name[:-len('_masked')]
        assert _lib.PROTOTYPES[name][0] is _lib.PROTOTYPES[unmasked][0]
        # the old argument list plus (mask, mask_row_stride)
        assert _lib.PROTOTYPES[name][1] == _lib.PROTOTYPES[unmasked][1] + [_lib.P, _lib.L]
    assert _lib.lib().kimg_version() == _lib.VERSION == 5


def test_unsupported_forms_with_a_mask_without_gpu():
    """The multi-component form, and the retired persistent and one-workgroup names, asked for
    with a mask: KIMG_EUNSUPPORTED,
    decided before any HIP call (there is no GPU here; the pointers are not device memory)."""
    from katsdpimager_amd import _lib
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)

    def call(form, mask, stride=64):
        return lib.kimg_clean_cycles_masked(p, p, 64, 4096, 64, 64, 1, p, 64, 4096, 64, 64, 33, 33, 2, 0,
                                            0.1, 0.0, p, p, 2, 2, 10, form, p, p, None, mask, stride)
    for form in (3, 4, 5, 5 | 3 << 8):      # KIMG_CLEAN_FORM_PERSISTENT, _ONE_WORKGROUP, _MULTI
        assert call(form, p) == -10002
    assert call(1, p, 10) == -10001         # rows of the mask shorter than the image's
    assert call(9, p) == -10001
    assert lib.kimg_update_tiles_masked(p, 64, 4096, 64, 64, 1, 2, 0, p, p, 2, 2, 0, 0, 2, 2, None,
                                        p, 10) == -10001


def test_process_channel_accepts_clean_mask():
    import inspect
    from katsdpimager_amd import clean, frontend, imaging
    sig = inspect.signature(frontend.process_channel)
    assert sig.parameters['clean_mask'].default is None
    assert callable(imaging.Imaging.set_clean_mask)

    class Slot:
        def __init__(self, buffer):
            self.buffer = buffer

    class Fake:
        """What batch_supported / multi_components look at."""
        def __init__(self, mask):
            self.slots = {'mask': Slot(mask), 'tile_max': Slot(np.zeros((8, 8), np.float32))}

        def buffer(self, name):
            return self.slots[name].buffer
    assert clean.batch_supported(Fake(None), (1, 33, 47)) and clean.multi_components(Fake(None), (1, 33, 47)) >= 2
    assert not clean.batch_supported(Fake(object()), (1, 33, 47))
    assert clean.multi_components(Fake(object()), (1, 33, 47)) == 0


# ---- GPU -----------------------------------------------------------------------------------------
G = 256
BORDER = 0.02           # 5 pixels: 246 candidates a side, 8 x 8 tiles
PATCH = (33, 47)        # 3 x 3 lattice blocks: the one-launch form runs
CYCLES = 200            # > KIMG_GRAPH_CYCLES (64): graph replays are covered
MASKS = ['ones', 'random50', 'random2', 'disks', 'no_brightest', 'empty_tiles', 'edge']


def problem(mode, P):
    rs, psf, dirty = sources_problem(100 * mode + P, G=G, P=P, n_sources=25)
    # sources next to the border and the image edge: their patches are clipped
    for y, x, amp in ((6, 100, 2.5), (250, 7, -2.2), (128, 249, 2.0), (5, 5, 1.8), (2, 60, 3.0)):
        dirty[:, y, x] += np.float32(amp)
    return psf, dirty


def brightest(dirty, mode, n):
    """(y, x) of the n highest metric values inside the border that are at least 12 pixels apart."""
    metric = np.abs(dirty[0]) if mode == 0 else np.sum(dirty * dirty, axis=0)
    inside = np.zeros_like(metric)
    inside[5:-5, 5:-5] = metric[5:-5, 5:-5]
    metric = inside
    out = []
    for _ in range(n):
        y, x = np.unravel_index(np.argmax(metric), metric.shape)
        out.append((int(y), int(x)))
        metric[max(0, y - 12):y + 13, max(0, x - 12):x + 13] = 0
    return out


def disk(y, x, r):
    yy, xx = np.mgrid[:G, :G]
    return (yy - y) ** 2 + (xx - x) ** 2 <= r * r


def make_mask(kind, dirty, mode):
    rs = np.random.RandomState(len(kind))
    if kind == 'ones':
        m = np.ones((G, G), bool)
    elif kind == 'zeros':
        m = np.zeros((G, G), bool)
    elif kind == 'random50':
        m = rs.uniform(size=(G, G)) < 0.5
    elif kind == 'random2':
        m = rs.uniform(size=(G, G)) < 0.02
    elif kind == 'disks':
        m = np.zeros((G, G), bool)
        for y, x in brightest(dirty, mode, 12):
            m |= disk(y, x, 6)
    elif kind == 'no_brightest':
        (y, x), = brightest(dirty, mode, 1)
        m = ~disk(y, x, 10)
    elif kind == 'empty_tiles':
        # whole tiles of the lattice (32 x 32 from the border) without an allowed pixel
        ty, tx = (np.mgrid[:G, :G] - 5) // 32
        m = (ty + tx) % 2 == 0
    elif kind == 'edge':
        # a frame that reaches the image edge: allowed pixels in the border (no candidates) and
        # candidates whose patches are clipped
        m = np.ones((G, G), bool)
        m[30:-30, 30:-30] = False
    else:
        raise ValueError(kind)
    return m.astype(np.uint8)


def make_clean(P, mode, dirty, psf, form, loop_gain=0.1):
    from helpers import context_queue
    from katsdpimager_amd import clean, parameters
    ctx, q = context_queue()
    fixed = parameters.FixedImageParameters(list(range(P)), np.float32)
    ip = parameters.ImageParameters(fixed, 1.0, None, 0.2, None, pixel_size=1e-5, pixels=G)
    cp = parameters.CleanParameters(1000, loop_gain, 0.85, 5.0, mode, 0.01, 0.5, BORDER)
    tuning = None if form in (None, 'per_call') else {'form': form}
    fn = clean.CleanTemplate(ctx, cp, np.float32, P, tuning).instantiate(q, ip)
    fn.ensure_all_bound()
    assert fn.buffer('mask') is None            # (optional: not bound by ensure_all_bound)
    fn.buffer('psf').set(q, psf)
    return fn, q


def device_mask(q, mask):
    from katsdpimager_amd import accel
    d = accel.DeviceArray(q.context, mask.shape, np.uint8, queue=q)
    d.set(q, np.ascontiguousarray(mask, np.uint8))
    return d


def start(fn, q, dirty, mask):
    fn.buffer('dirty').set(q, dirty)
    fn.buffer('model').zero(q)
    fn.bind(mask=None if mask is None else device_mask(q, mask))
    fn.reset()


def run(fn, q, form, patch, threshold, cycles):
    if form == 'per_call':
        log = []
        for _ in range(cycles):
            v, pos, pix = fn(patch, threshold)
            if v is None:
                break
            log.append((v, pos, pix))
    else:
        log = fn.run_cycles(patch, threshold, cycles)
    return (log, fn.buffer('dirty').get(q), fn.buffer('model').get(q), fn.buffer('tile_max').get(q),
            fn.buffer('tile_pos').get(q))


@gpu
@pytest.mark.parametrize('kind', MASKS)
@pytest.mark.parametrize('mode,P', [(0, 1), (1, 1), (0, 4), (1, 4), (0, 2), (1, 2), (0, 3), (1, 3)])
def test_masked_forms_vs_restatement(mode, P, kind):
    """200 cycles on 256^2 under every mask, in the per-call, two-launch and one-launch forms (and
    what `auto` takes with a mask): all of it the restatement's, bit for bit."""
    psf, dirty = problem(mode, P)
    mask = make_mask(kind, dirty, mode)
    patch = (P,) + PATCH
    want = masked_run(G, BORDER, 0.1, mode, dirty, psf, patch, 0.0, CYCLES, mask)
    assert len(want[0]) == CYCLES                               # (no case ends early or is skipped)
    assert all(mask[pos] for _, pos, _ in want[0])
    assert set(zip(*np.nonzero(np.any(want[2] != 0, axis=0)))) <= set(zip(*np.nonzero(mask)))
    if kind == 'ones':
        same_run(want, plain_run(G, BORDER, 0.1, mode, dirty, psf, patch, 0.0, CYCLES))
    if kind in ('empty_tiles', 'disks', 'edge'):
        assert np.any(want[3] == 0)                             # tiles without a candidate
    if kind == 'no_brightest':
        top = plain_run(G, BORDER, 0.1, mode, dirty, psf, patch, 0.0, 1)[0][0][1]
        assert not mask[top] and all((y - top[0]) ** 2 + (x - top[1]) ** 2 > 100 for _, (y, x), _ in want[0])
    if kind == 'edge':
        clipped = [pos for _, pos, _ in want[0]
                   if pos[0] < PATCH[0] // 2 or pos[1] < PATCH[1] // 2
                   or pos[0] >= G - PATCH[0] // 2 or pos[1] >= G - PATCH[1] // 2]
        assert len(clipped) >= 3
    for form in ('per_call', 'two_launch', 'one_launch', 'auto'):
        fn, q = make_clean(P, mode, dirty, psf, form)
        start(fn, q, dirty, mask)
        same_run(run(fn, q, form, patch, 0.0, CYCLES), want)
        if form != 'per_call':
            assert fn.last_launches() is None                   # (not the multi-component form)
    if kind == 'ones':
        # ... and the all-ones mask is the unmasked run, in the form that takes without a mask
        fn, q = make_clean(P, mode, dirty, psf, 'auto')
        start(fn, q, dirty, None)
        same_run(run(fn, q, 'auto', patch, 0.0, CYCLES), want)
        assert fn.last_launches() is not None


@gpu
@pytest.mark.parametrize('mode,P', [(0, 1), (1, 4)])
def test_all_zero_mask_stops_at_once(mode, P):
    psf, dirty = problem(mode, P)
    patch = (P,) + PATCH
    mask = make_mask('zeros', dirty, mode)
    for form in ('per_call', 'two_launch', 'one_launch', 'auto'):
        fn, q = make_clean(P, mode, dirty, psf, form)
        start(fn, q, dirty, mask)
        assert not np.any(fn.buffer('tile_max').get(q))
        if form == 'per_call':
            assert fn(patch, 0.0) == (None, None, None)         # even at threshold 0
        else:
            assert fn.run_cycles(patch, 0.0, 100) == []
        np.testing.assert_array_equal(fn.buffer('dirty').get(q), dirty)
        assert not np.any(fn.buffer('model').get(q))
        # the same buffers without the mask place components again (metric 0 would too: unchanged)
        fn.bind(mask=None)
        fn.reset()
        assert len(run(fn, q, form, patch, 0.0, 3)[0]) == 3


@gpu
def test_mask_runs_dry_then_stops():
    """A mask whose allowed pixels are all cleaned to exactly 0 (loop gain 1, a one-pixel PSF patch):
    the loop takes them one by one and then stops at metric 0, below any threshold."""
    P, mode = 1, 0
    psf, dirty = problem(mode, P)
    mask = np.zeros((G, G), np.uint8)
    spots = [(40, 50), (41, 50), (120, 200), (200, 33), (201, 34)]
    for s in spots:
        mask[s] = 1
    patch = (1, 1, 1)
    want = masked_run(G, BORDER, 1.0, mode, dirty, psf, patch, 0.0, 50, mask)
    assert len(want[0]) == len(spots)
    for form in ('per_call', 'two_launch', 'one_launch'):
        fn, q = make_clean(P, mode, dirty, psf, form, loop_gain=1.0)
        start(fn, q, dirty, mask)
        same_run(run(fn, q, form, patch, 0.0, 50), want)


@gpu
@pytest.mark.parametrize('mode,P', [(0, 1), (1, 4), (1, 3)])
def test_threshold_stop_under_a_mask(mode, P):
    psf, dirty = problem(mode, P)
    patch = (P,) + PATCH
    mask = make_mask('random50', dirty, mode)
    ref = MaskedClean(G, BORDER, 0.1, mode, dirty.copy(), psf, np.zeros_like(dirty), mask)
    ref.reset()
    first = float(np.max(ref._tile_max))
    threshold = (0.45 if mode == 0 else 0.2) * first
    want = masked_run(G, BORDER, 0.1, mode, dirty, psf, patch, threshold, 500, mask)
    assert 10 < len(want[0]) < 500
    for form in ('per_call', 'two_launch', 'one_launch'):
        fn, q = make_clean(P, mode, dirty, psf, form)
        start(fn, q, dirty, mask)
        same_run(run(fn, q, form, patch, threshold, 500), want)
    # consecutive calls continue where the last one stopped
    fn, q = make_clean(P, mode, dirty, psf, 'auto')
    start(fn, q, dirty, mask)
    for cycles, thr in ((1, 0.0), (3, 0.0), (70, 0.0), (500, threshold), (40, 0.0)):
        got = fn.run_cycles(patch, thr, cycles)
        want = masked_run(None, None, None, None, None, None, patch, thr, cycles, None, ref=ref)
        same_run((got, fn.buffer('dirty').get(q), fn.buffer('model').get(q),
                  fn.buffer('tile_max').get(q), fn.buffer('tile_pos').get(q)), want)


@gpu
@pytest.mark.parametrize('form', ['two_launch', 'one_launch'])
def test_two_masks_in_turn_do_not_share_a_graph(form):
    """The same images, tile arrays, state and log under two masks in turn (two device arrays, then
    one device array rewritten in place): every run is its own mask's."""
    P, mode = 1, 0
    psf, dirty = problem(mode, P)
    patch = (P,) + PATCH
    masks = [make_mask(k, dirty, mode) for k in ('random50', 'disks', 'empty_tiles')]
    wants = [masked_run(G, BORDER, 0.1, mode, dirty, psf, patch, 0.0, CYCLES, m) for m in masks]
    fn, q = make_clean(P, mode, dirty, psf, form)
    devices = [device_mask(q, m) for m in masks[:2]]
    for i in (0, 1, 0, 1):
        fn.buffer('dirty').set(q, dirty)
        fn.buffer('model').zero(q)
        fn.bind(mask=devices[i])
        fn.reset()
        same_run(run(fn, q, form, patch, 0.0, CYCLES), wants[i])
    for i in (2, 0, 1):
        devices[0].set(q, masks[i])
        fn.buffer('dirty').set(q, dirty)
        fn.buffer('model').zero(q)
        fn.bind(mask=devices[0])
        fn.reset()
        same_run(run(fn, q, form, patch, 0.0, CYCLES), wants[i])
    # ... and without a mask on the same buffers again
    start(fn, q, dirty, None)
    same_run(run(fn, q, form, patch, 0.0, CYCLES), plain_run(G, BORDER, 0.1, mode, dirty, psf, patch, 0.0, CYCLES))


@gpu
def test_unmasked_runs_take_the_forms_they_took():
    """No mask bound: `auto` takes the multi-component form and the batch launch is available, as
    before; with a mask neither is, the forms without masked kernels refuse, and a batcher runs the
    channel on its own."""
    from katsdpimager_amd import _lib, clean
    P, mode = 1, 0
    psf, dirty = problem(mode, P)
    patch = (P,) + PATCH
    mask = make_mask('random50', dirty, mode)
    want = masked_run(G, BORDER, 0.1, mode, dirty, psf, patch, 0.0, CYCLES, mask)
    plain = plain_run(G, BORDER, 0.1, mode, dirty, psf, patch, 0.0, CYCLES)
    fn, q = make_clean(P, mode, dirty, psf, None)
    start(fn, q, dirty, None)
    assert clean.batch_supported(fn, patch) and clean.multi_components(fn, patch) >= 2
    assert clean.prefers_solo(fn, patch, CYCLES)
    same_run(run(fn, q, 'auto', patch, 0.0, CYCLES), plain)
    launches = fn.last_launches()
    assert launches is not None and launches < CYCLES           # several components per launch
    start(fn, q, dirty, None)
    done, first = fn.run_major_cycles(patch, 0.0, 0.0, 50)
    assert done == 50 and first == plain[0][0][0]
    assert fn.last_launches() is not None
    # with a mask
    start(fn, q, dirty, mask)
    assert not clean.batch_supported(fn, patch) and clean.multi_components(fn, patch) == 0
    assert not clean.prefers_solo(fn, patch, CYCLES)
    assert not fn.run_major_cycles(patch, 0.0, 0.0, 50)
    np.testing.assert_array_equal(fn.buffer('dirty').get(q), dirty)        # (it did nothing)
    batcher = clean.CleanBatcher(1)
    assert batcher.run_major_cycles(fn, patch, 0.0, 0.0, 50) is None
    got = batcher.run_cycles(fn, patch, 0.0, CYCLES)
    assert batcher.batches == []
    same_run((got, fn.buffer('dirty').get(q), fn.buffer('model').get(q),
              fn.buffer('tile_max').get(q), fn.buffer('tile_pos').get(q)), want)
    assert fn.last_launches() is None
    with pytest.raises(ValueError):
        fn.bind(mask=device_mask(q, np.ones((G, G + 1), np.uint8)))
    for form in ('multi', 'persistent', 'one_workgroup'):
        other, q = make_clean(P, mode, dirty, psf, form)
        start(other, q, dirty, mask)
        with pytest.raises(_lib.KimgError) as err:
            other.run_cycles(patch, 0.0, CYCLES)
        assert err.value.code == -10002                         # KIMG_EUNSUPPORTED
    # the mask taken off: the multi-component form again, the unmasked result
    start(fn, q, dirty, None)
    same_run(run(fn, q, 'auto', patch, 0.0, CYCLES), plain)
    assert fn.last_launches() is not None and fn.last_launches() < CYCLES


# ---- GPU: the driver -------------------------------------------------------------------------------
def _channel(c):
    from helpers import context_queue, make_params
    from katsdpimager_amd import parameters, preprocess, weight
    ctx, q = context_queue()
    ip, gp, ap = make_params(c)
    wp = parameters.WeightParameters(weight.WeightType(c['weight_type']), c['robustness'])
    cp = parameters.CleanParameters(c['minor'], c['loop_gain'], c['major_gain'], c['threshold'],
                                    c['mode'], c['psf_cutoff'], c['psf_limit'], c['border'])
    uvw, vis, weights = gi.e2e_raw(c)
    vis = vis[:, None] if vis.ndim == 1 else vis
    coll = preprocess.VisibilityCollectorDevice(q, [ip], [gp], max(len(uvw), c['vis_block']))
    coll.add(uvw, weights[None], vis[None].astype(np.complex64), None, None,
             np.identity(c['P'], dtype=np.complex64), None)
    coll.close()
    return ctx, q, ip, gp, ap, wp, cp, coll.reader()


@gpu
@pytest.mark.parametrize('name', ['degrid', 'stokes'])
def test_process_channel_with_clean_mask(name):
    """frontend.process_channel(clean_mask=...) on the synthetic channel of the end-to-end tests
    (the recipe of test_preprocess_gpu.test_store_driven_channel_vs_golden).

    Every component lies in the mask, and none where the mask forbids the unmasked run's first
    component.  With an all-ones mask the driver gives what it gives with clean_mask=None on the
    same path (first cycle on its own, the rest in one device-resident loop): the same component
    positions and cycle counts exactly; the images to the bounds that test sets for two runs of one
    driver, whose gridders' float atomics differ in the last bits from run to run (tapered dirty
    1e-5, inner dirty 1e-4, model 1e-5)."""
    from helpers import kernel_taper, relerr, tapered_relerr
    from katsdpimager_amd import frontend, imaging
    c = gi.E2E_CONFIGS[name]
    ctx, q, ip, gp, ap, wp, cp, reader = _channel(c)
    pixels = c['pixels']

    def drive(mask, one_call):
        im = imaging.ImagingTemplate(ctx, ap, ip.fixed, wp, gp.fixed, cp).instantiate(
            q, ip, gp, c['vis_block'], 0, c['major'])
        im.ensure_all_bound()
        if not one_call:
            im.one_call_major_cycles = False
        stats = frontend.process_channel(reader, 0, im, ip, gp, cp, wp.weight_type, c['vis_block'],
                                         c['major'], c['degrid'], clean_mask=mask)
        assert im.clean_mask is None            # (the mask was this call's only)
        return stats, im.get_buffer('dirty'), im.get_buffer('model'), dict(im._model_components)

    s0, d0, m0, c0 = drive(None, False)
    s1, d1, m1, c1 = drive(np.ones((pixels, pixels), bool), True)
    assert s0['minor'] == s1['minor'] > 0 and s0['major'] == s1['major'] == c['major']
    assert s0['psf_patch'] == s1['psf_patch']
    assert sorted(c0) == sorted(c1)
    taper = kernel_taper(c)
    inner = np.s_[:, pixels // 8:-pixels // 8, pixels // 8:-pixels // 8]
    assert tapered_relerr(d1, d0, taper) < 1e-5 and relerr(d1[inner], d0[inner]) < 1e-4
    assert relerr(m1, m0) < 1e-5
    # a mask that forbids the neighbourhood of the strongest component
    power = {pos: float(np.sum(np.square(v))) for pos, v in c0.items()}
    y, x = max(power, key=power.get)
    mask = ~((np.mgrid[:pixels, :pixels][0] - y) ** 2 + (np.mgrid[:pixels, :pixels][1] - x) ** 2 <= 64)
    s2, d2, m2, c2 = drive(mask.astype(np.uint8), True)
    assert s2['minor'] > 0 and len(c2) > 0
    assert all(mask[pos] for pos in c2)
    assert set(zip(*np.nonzero(np.any(m2 != 0, axis=0)))) <= set(zip(*np.nonzero(mask)))
    assert (y, x) not in c2
    # nothing allowed: no component, no cycle counted, and the driver returns
    s3, d3, m3, c3 = drive(np.zeros((pixels, pixels), np.uint8), True)
    assert c3 == {} and s3['minor'] == 0 and not np.any(m3)
