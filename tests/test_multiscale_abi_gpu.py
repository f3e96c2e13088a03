"""Multi-scale CLEAN through the C ABI (csrc/clean_scales.hip) on non-square, padded, offset and wide
images, against its numpy twin: the convolution past one workgroup along x, the set-up and the
cycles of every case of tests/multiscale_cases.py under every buffer layout, masks with a pitch of
their own, the stopping rule at equality, the residuals-only set-up and the all-zero image.  Every
comparison is exact.  tests/test_multiscale_cases_host.py shows which branch of the kernels each
case reaches under which layout."""
import numpy as np
import pytest

import multiscale_cases as mc
from helpers import Padded, context_queue

from katsdpimager_amd import multiscale as ms

gpu = pytest.mark.gpu

CASE_LAYOUTS = [(name, layout) for name in mc.CASES for layout in mc.LAYOUTS]


# ---- the convolution, more than one workgroup along x -----------------------------------------------

@gpu
@pytest.mark.parametrize('shape', [(40, 257), (33, 520)])
@pytest.mark.parametrize('R', [0, 1, 64])
def test_convolve_wide(shape, R):
    from katsdpimager_amd import accel
    from katsdpimager_amd._lib import lib, check
    ctx, q = context_queue()
    H, W = shape
    P = 2
    rng = np.random.default_rng(R * 1000 + W)
    x = rng.standard_normal((P, H, W)).astype(np.float32)
    taps = rng.standard_normal(2 * R + 1).astype(np.float32)
    aa = np.frombuffer(b'\xaa' * 4, np.float32)[0]
    src = Padded(ctx, q, x, rpad=5, vpad=2, sentinel=aa, origin=(0, 3))
    tmp = Padded(ctx, q, np.full_like(x, aa), rpad=1, vpad=0, sentinel=aa, origin=(0, 3))
    out = Padded(ctx, q, np.full_like(x, aa), rpad=9, vpad=1, sentinel=aa, origin=(0, 3))
    dtaps = accel.DeviceArray(ctx, taps.shape, np.float32, queue=q)
    dtaps.set(q, taps)
    check(lib().kimg_image_convolve_separable(
        src.ptr, src.row, src.pol, out.ptr, out.row, out.pol, tmp.ptr, tmp.row, tmp.pol,
        W, H, P, dtaps.ptr, R, q.handle), 'kimg_image_convolve_separable')
    np.testing.assert_array_equal(tmp.get(q), ms._conv_axis(x, taps))       # (.get checks the padding)
    np.testing.assert_array_equal(out.get(q), ms.conv_host(x, taps))
    np.testing.assert_array_equal(src.get(q), x)


# ---- set-up -------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('name,layout', CASE_LAYOUTS)
def test_setup_through_the_abi(name, layout):
    c = mc.CASES[name]
    ctx, q = context_queue()
    twin, setup, log = c.reference()
    b = mc.Bound(ctx, q, c, layout)
    b.setup()
    ws = b.read_workspace()                                 # (checks the guard)
    n, inv = b.norms(ws)
    np.testing.assert_array_equal(n, twin.norms)
    np.testing.assert_array_equal(inv, twin.inv)
    assert n[0] == 1 and inv[0] == 1
    for j in range(c.K):
        for k in range(c.K):
            X = b.cross_patch(ws, j, k)
            R = c.params.radii[j] + c.params.radii[k]
            assert X.shape == (c.P, min(c.patch[1] + 2 * R, c.H), min(c.patch[2] + 2 * R, c.W))
            np.testing.assert_array_equal(X, twin.cross[j, k], 'X %d %d' % (j, k))
    for k in range(c.K):
        np.testing.assert_array_equal(b.residual(ws, k), setup['residuals'][k], 'residual %d' % k)
    tmax, tpos = b.tile_records(ws)
    np.testing.assert_array_equal(tmax, setup['tile_max'])
    np.testing.assert_array_equal(tpos, setup['tile_pos'])
    np.testing.assert_array_equal(b.model.get(q), 0)
    b.assert_inputs_untouched()


# ---- cycles -------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('name,layout', CASE_LAYOUTS)
def test_cycles_through_the_abi(name, layout):
    c = mc.CASES[name]
    ctx, q = context_queue()
    twin, setup, want = c.reference()
    b = mc.Bound(ctx, q, c, layout)
    b.setup()
    got = b.cycles(0.0, c.cycles)
    assert b.cycles_done == len(want) == c.cycles
    mc.same_log(got, want)
    b.assert_state(twin)


_masked = {}


def _masked_reference(name):
    if name not in _masked:
        c = mc.CASES[name]
        mask = mc.blocky_mask(c)
        twin = c.twin(mask=mask)
        _masked[name] = (mask, twin, twin.run_cycles(c.patch, 0.0, c.cycles))
    return _masked[name]


@gpu
@pytest.mark.parametrize('layout', mc.LAYOUTS)
@pytest.mark.parametrize('name', ['wide', 'tall'])
def test_cycles_with_a_padded_mask(name, layout):
    c = mc.CASES[name]
    ctx, q = context_queue()
    mask, twin, want = _masked_reference(name)
    assert len(want) == c.cycles and np.all(mask[want['y'], want['x']])
    assert 0 < mask.sum() < mask.size
    b = mc.Bound(ctx, q, c, layout, mask=mask)
    b.setup()
    got = b.cycles(0.0, c.cycles)
    mc.same_log(got, want)
    assert np.all(mask[got['y'], got['x']])
    b.assert_state(twin)
    # nothing allowed: no component whatever the threshold (the mask's padding is 1 = allowed)
    none = np.zeros((c.H, c.W), bool)
    twin0 = c.twin(mask=none)
    assert len(twin0.run_cycles(c.patch, 0.0, 10)) == 0
    b0 = mc.Bound(ctx, q, c, layout, mask=none)
    b0.setup()
    assert len(b0.cycles(0.0, 10)) == 0 and b0.cycles_done == 0
    b0.assert_state(twin0)


# ---- the stopping rule at equality ------------------------------------------------------------------

def _stop_cycles(later):
    """A cycle n of `wide` whose peak is below every earlier one, so that the threshold peaks[n] is
    met first at n: the last such cycle whose winning scale is not 0, or (``later``) the first one
    with n > 64 inside a chunk, whatever its scale."""
    c = mc.CASES['wide']
    log = c.reference()[2]
    peaks = log['peak']
    lowest = [n for n in range(1, len(log)) if peaks[n] < peaks[:n].min()]
    if later:
        ok = [n for n in lowest if n > 64 and n % 64 != 0]
    else:
        ok = [n for n in lowest if log['scale'][n] >= 1][-1:]
    assert ok, 'no such cycle: change the case'
    return ok[0]


@gpu
@pytest.mark.parametrize('layout', ['compact', 'pitch+1'])
@pytest.mark.parametrize('later', [False, True])
def test_threshold_equal_to_the_peak_takes_the_component(later, layout):
    """The rule is peak < threshold on the unbiased peak of the scale that won on the biased one:
    a threshold equal to that peak takes the component, the next float above it does not."""
    c = mc.CASES['wide']
    ctx, q = context_queue()
    n = _stop_cycles(later)
    log = c.reference()[2]
    assert later or log['scale'][n] >= 1
    peak = log['peak'][n]
    for threshold, exactly in ((float(peak), None), (float(np.nextafter(peak, np.float32(np.inf))), n)):
        twin = c.twin()
        want = twin.run_cycles(c.patch, threshold, c.cycles)
        b = mc.Bound(ctx, q, c, layout)
        b.setup()
        got = b.cycles(threshold, c.cycles)
        mc.same_log(got, want)
        assert b.cycles_done == len(got)
        if exactly is None:
            assert len(got) >= n + 1
            mc.same_log(got[n:n + 1], log[n:n + 1])
            assert got['peak'][n] == np.float32(threshold)
        else:
            assert len(got) == exactly
            mc.same_log(got, log[:n])
        b.assert_state(twin)


# ---- the residuals-only set-up ----------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('layout', ['compact', 'pitch+1', 'offset'])
def test_residuals_only_setup_after_a_new_dirty_image(layout):
    c = mc.CASES['wide']
    ctx, q = context_queue()
    second = mc.field(c.H, c.W, c.P, c.bp, c.seed + 100, None)[0]
    psf = c.field()[1]
    first = c.twin()
    want1 = first.run_cycles(c.patch, 0.0, 30)
    twin = c.twin(dirty=second.copy(), model=first.model.copy())
    want2 = twin.run_cycles(c.patch, 0.0, 30)
    assert len(want1) == len(want2) == 30

    b = mc.Bound(ctx, q, c, layout)
    b.setup()
    mc.same_log(b.cycles(0.0, 30), want1)
    ws = b.assert_state(first)
    cross = {jk: b.cross_patch(ws, *jk).copy() for jk in b.lay['cross']}
    norms = b.norms(ws)
    whole = b.dirty.dev.get(q)
    whole[b.dirty.inside] = second
    b.dirty.dev.set(q, whole)
    b.setup(mc.SETUP_RESIDUALS)
    ws = b.read_workspace()
    for k in range(1, c.K):
        np.testing.assert_array_equal(
            b.residual(ws, k), ms.conv_host(second, c.params.taps[k]) * first.inv[k])
    mc.same_log(b.cycles(0.0, 30), want2)
    ws = b.assert_state(twin)
    for jk, X in cross.items():
        np.testing.assert_array_equal(b.cross_patch(ws, *jk).view(np.uint32), X.view(np.uint32))
    for before, after in zip(norms, b.norms(ws)):
        np.testing.assert_array_equal(before, after)
    np.testing.assert_array_equal(b.psf.get(q), psf)


# ---- the all-zero image -----------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('layout', mc.LAYOUTS)
def test_all_zero_image_without_a_mask(layout):
    """Threshold 0 and no mask: every cycle takes a component of zero flux at the first tile's
    start position, and nothing outside the interior is written."""
    c = mc.CASES['tiny']
    ctx, q = context_queue()
    zero = np.zeros((c.P, c.H, c.W), np.float32)
    twin = c.twin(dirty=zero.copy())
    want = twin.run_cycles(c.patch, 0.0, c.cycles)
    assert len(want) == c.cycles
    assert np.all(want['y'] == c.bp) and np.all(want['x'] == c.bp) and np.all(want['scale'] == 0)
    assert np.all(want['peak'] == 0) and np.all(want['flux'] == 0)
    b = mc.Bound(ctx, q, c, layout, dirty=zero)
    b.setup()
    got = b.cycles(0.0, c.cycles)
    mc.same_log(got, want)
    assert b.cycles_done == c.cycles
    b.assert_state(twin)
    np.testing.assert_array_equal(b.model.get(q), 0)
