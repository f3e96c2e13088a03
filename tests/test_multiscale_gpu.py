"""Multi-scale CLEAN on the device (csrc/clean_scales.hip) against its numpy twin
(multiscale.MultiScaleCleanHost): the separable convolution, the set-up, the minor cycles, the
single scale 0 against the Hogbom loop, and the driver.  Every comparison with the twin is exact.
Set-up and cycles run at 1, 2, 3 and 4 polarizations (DESIGN.md 5.17 lists which test launches which
entry point of the library at which count)."""
import numpy as np
import pytest

import golden_inputs as gi
from helpers import Padded, context_queue

from katsdpimager_amd import multiscale as ms
from katsdpimager_amd.parameters import CLEAN_I

gpu = pytest.mark.gpu


def _params(G, P, border, loop_gain):
    from katsdpimager_amd import parameters
    fixed = parameters.FixedImageParameters(list(range(P)), np.float32)
    ip = parameters.ImageParameters(fixed, 1.0, None, 0.2, None, pixel_size=1e-5, pixels=G)
    cp = parameters.CleanParameters(1000, loop_gain, 0.85, 5.0, CLEAN_I, 0.01, 0.5, border)
    return ip, cp


def field(G, P, border, seed, noise=0.05):
    """(dirty, psf): noise plus blobs and points, some of them 3 pixels inside the border on every
    side, so that boxes clip at all four edges; a Gaussian-core PSF with noisy wings, centre 1."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:G, :G].astype(np.float64)
    c = G // 2
    psf = np.empty((P, G, G), np.float32)
    for p in range(P):
        psf[p] = np.exp(-((yy - c) ** 2 + (xx - c) ** 2) / (2 * 1.7 ** 2)) \
            + 0.01 * rng.standard_normal((G, G))
    psf /= psf[:, c, c][:, None, None]
    assert np.all(psf[:, c, c] == 1)
    dirty = noise * rng.standard_normal((P, G, G))
    bp = round(border * G)
    lo, hi = bp + 3, G - bp - 4
    for (y, x, fwhm, amp) in [(lo, lo, 6, 6.0), (lo, hi, 0, -4.0), (hi, lo, 3, 5.0), (hi, hi, 8, -7.0),
                              (c, lo, 0, 3.0), (c + 5, c - 9, 9, 8.0), (hi, c, 4, 4.0)]:
        s = max(fwhm, 1.0) / 2.355
        blob = amp * np.exp(-((yy - y) ** 2 + (xx - x) ** 2) / (2 * s * s))
        for p in range(P):
            dirty[p] += blob * (1.0 - 0.3 * p)
    return dirty.astype(np.float32), psf


def make_op(G, P, scales, border, loop_gain, dirty, psf, mask=None, biases=None):
    from katsdpimager_amd import accel
    ctx, q = context_queue()
    ip, cp = _params(G, P, border, loop_gain)
    params = ms.MultiScaleParameters(scales, biases)
    op = ms.MultiScaleCleanTemplate(ctx, cp, params, np.float32, P).instantiate(q, ip)
    op.ensure_all_bound()
    op.buffer('dirty').set(q, dirty)
    op.buffer('psf').set(q, psf)
    op.buffer('model').zero(q)
    if mask is not None:
        dm = accel.DeviceArray(ctx, mask.shape, np.uint8, queue=q)
        dm.set(q, mask.astype(np.uint8))
        op.bind(mask=dm)
    twin = ms.MultiScaleCleanHost(params, border, loop_gain, CLEAN_I, dirty.copy(), psf,
                                  np.zeros_like(dirty), mask=mask)
    return op, twin, q


def same_state(op, twin, q):
    K = len(twin.params)
    for k in range(K):
        np.testing.assert_array_equal(op.residual(k), twin.residuals[k], 'residual %d' % k)
    np.testing.assert_array_equal(op.buffer('model').get(q), twin.model)
    tmax, tpos = op.tile_records()
    np.testing.assert_array_equal(tmax, twin.tile_max)
    np.testing.assert_array_equal(tpos, twin.tile_pos)


def same_log(got, want):
    assert len(got) == len(want)
    for name in ('scale', 'y', 'x', 'peak', 'flux'):
        np.testing.assert_array_equal(got[name], want[name], name)


# ---- the convolution ------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('shape', [(40, 70), (33, 200)])
@pytest.mark.parametrize('R', [0, 1, 7, 31, 64])
def test_convolve_matches_twin(shape, R):
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
    want_tmp = ms._conv_axis(x, taps)
    np.testing.assert_array_equal(tmp.get(q), want_tmp)             # (.get checks the padding)
    np.testing.assert_array_equal(out.get(q), ms.conv_host(x, taps))
    np.testing.assert_array_equal(src.get(q), x)


@gpu
@pytest.mark.parametrize('P', [1, 3, 4])
def test_convolve_matches_twin_pols(P):
    """test_convolve_matches_twin (which runs P = 2) at the other counts, on the narrow shape with
    the radii 7 and 64: every plane is its own convolution, through its own pitch."""
    from katsdpimager_amd import accel
    from katsdpimager_amd._lib import lib, check
    ctx, q = context_queue()
    H, W = 33, 200
    aa = np.frombuffer(b'\xaa' * 4, np.float32)[0]
    for R in (7, 64):
        rng = np.random.default_rng(R * 1000 + W + P)
        x = rng.standard_normal((P, H, W)).astype(np.float32)
        taps = rng.standard_normal(2 * R + 1).astype(np.float32)
        src = Padded(ctx, q, x, rpad=5, vpad=2, sentinel=aa, origin=(0, 3))
        tmp = Padded(ctx, q, np.full_like(x, aa), rpad=1, vpad=0, sentinel=aa, origin=(0, 3))
        out = Padded(ctx, q, np.full_like(x, aa), rpad=9, vpad=1, sentinel=aa, origin=(0, 3))
        dtaps = accel.DeviceArray(ctx, taps.shape, np.float32, queue=q)
        dtaps.set(q, taps)
        check(lib().kimg_image_convolve_separable(
            src.ptr, src.row, src.pol, out.ptr, out.row, out.pol, tmp.ptr, tmp.row, tmp.pol,
            W, H, P, dtaps.ptr, R, q.handle), 'kimg_image_convolve_separable')
        np.testing.assert_array_equal(tmp.get(q), ms._conv_axis(x, taps))
        np.testing.assert_array_equal(out.get(q), ms.conv_host(x, taps))
        np.testing.assert_array_equal(src.get(q), x)


# ---- set-up ---------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('P', [1, 2, 3, 4])
def test_setup_matches_twin(P):
    G, border, patch = 96, 0.02, (P, 15, 17)
    dirty, psf = field(G, P, border, 7 + P)
    op, twin, q = make_op(G, P, [0, 4, 9], border, 0.1, dirty, psf)
    op.reset()
    op.prepare(patch)
    twin.reset()
    twin.prepare(patch)
    n, inv = op.scale_norms()
    np.testing.assert_array_equal(n, twin.norms)
    np.testing.assert_array_equal(inv, twin.inv)
    assert n[0] == 1 and inv[0] == 1
    for j in range(3):
        for k in range(3):
            X = op.cross_patch(j, k)
            assert X.shape == (P, 15 + 2 * (twin.params.radii[j] + twin.params.radii[k]),
                               17 + 2 * (twin.params.radii[j] + twin.params.radii[k]))
            np.testing.assert_array_equal(X, twin.cross[j, k], 'X %d %d' % (j, k))
    same_state(op, twin, q)


# ---- cycles ---------------------------------------------------------------------------------------

CYCLES = 200


def _run_both(op, twin, q, patch, threshold, cycles=CYCLES):
    op.reset()
    twin.reset()
    got = op.run_cycles(patch, threshold, cycles)
    want = twin.run_cycles(patch, threshold, cycles)
    same_log(got, want)
    assert op.cycles_done == len(want)
    same_state(op, twin, q)
    return got


@gpu
@pytest.mark.parametrize('P', [1, 2, 3, 4])
def test_cycles_clipped_on_all_sides(P):
    """Threshold 0, noise plus blobs 3 pixels from the border: boxes clip on all four sides."""
    G, border, patch = 96, 0.02, (P, 15, 17)
    dirty, psf = field(G, P, border, 21)
    op, twin, q = make_op(G, P, [0, 4, 9], border, 0.1, dirty, psf)
    log = _run_both(op, twin, q, patch, 0.0)
    assert len(log) == CYCLES
    assert len(set(log['scale'].tolist())) == 3                     # every scale is taken
    R = np.array(twin.params.radii)[log['scale']] * 2 + 7
    assert np.any(log['y'] - R < 0) and np.any(log['y'] + R >= G)
    assert np.any(log['x'] - R < 0) and np.any(log['x'] + R >= G)


@gpu
def test_cycles_stop_mid_chunk():
    """A threshold met inside a chunk of 64: the count is exact and nothing is subtracted after."""
    G, P, border, patch = 96, 1, 0.02, (1, 15, 17)
    dirty, psf = field(G, P, border, 22)
    op, twin, q = make_op(G, P, [0, 4, 9], border, 0.1, dirty, psf)
    probe = ms.MultiScaleCleanHost(twin.params, border, 0.1, CLEAN_I, dirty.copy(), psf,
                                   np.zeros_like(dirty))
    peaks = probe.run_cycles(patch, 0.0, 150)['peak']
    threshold = float(np.nextafter(peaks[100], np.float32(np.inf)))
    log = _run_both(op, twin, q, patch, threshold)
    assert 0 < len(log) < CYCLES and len(log) % 64 != 0
    assert np.all(log['peak'] >= np.float32(threshold))


@gpu
@pytest.mark.parametrize('P', [4])
def test_cycles_stop_mid_chunk_pols(P):
    """test_cycles_stop_mid_chunk (which runs P = 1) at four polarizations: the count is exact, the
    last component's four fluxes end the log and nothing is subtracted from any plane after it.
    P = 2 and 3 take no other code: the stopping rule reads polarization 0 alone, and a cycle's
    per-polarization work runs at every count in test_cycles_clipped_on_all_sides."""
    G, border, patch = 96, 0.02, (P, 15, 17)
    dirty, psf = field(G, P, border, 22)
    op, twin, q = make_op(G, P, [0, 4, 9], border, 0.1, dirty, psf)
    probe = ms.MultiScaleCleanHost(twin.params, border, 0.1, CLEAN_I, dirty.copy(), psf,
                                   np.zeros_like(dirty))
    peaks = probe.run_cycles(patch, 0.0, 150)['peak']
    threshold = float(np.nextafter(peaks[100], np.float32(np.inf)))
    log = _run_both(op, twin, q, patch, threshold)
    assert 0 < len(log) < CYCLES and len(log) % 64 != 0
    assert np.all(log['peak'] >= np.float32(threshold))
    assert log['flux'].shape == (len(log), P)


@gpu
def test_cycles_with_mask():
    G, P, border, patch = 96, 2, 0.02, (2, 15, 17)
    dirty, psf = field(G, P, border, 23)
    rng = np.random.default_rng(5)
    mask = np.kron(rng.random((12, 12)) < 0.4, np.ones((8, 8), bool))
    mask[:, 40:44] = True
    op, twin, q = make_op(G, P, [0, 4, 9], border, 0.1, dirty, psf, mask=mask)
    log = _run_both(op, twin, q, patch, 0.0)
    assert len(log) == CYCLES
    assert np.all(mask[log['y'], log['x']])
    # nothing allowed: no component whatever the threshold
    op2, twin2, q = make_op(G, P, [0, 4, 9], border, 0.1, dirty, psf, mask=np.zeros((G, G), bool))
    assert len(_run_both(op2, twin2, q, patch, 0.0, 10)) == 0


@gpu
@pytest.mark.parametrize('P', [3, 4])
def test_cycles_with_mask_pols(P):
    """test_cycles_with_mask (which runs P = 2) at three and four polarizations.  P = 1 under a mask
    takes no other code: the mask enters through is_candidate alone, which does not see the count."""
    G, border, patch = 96, 0.02, (P, 15, 17)
    dirty, psf = field(G, P, border, 23)
    rng = np.random.default_rng(5)
    mask = np.kron(rng.random((12, 12)) < 0.4, np.ones((8, 8), bool))
    mask[:, 40:44] = True
    op, twin, q = make_op(G, P, [0, 4, 9], border, 0.1, dirty, psf, mask=mask)
    log = _run_both(op, twin, q, patch, 0.0)
    assert len(log) == CYCLES
    assert np.all(mask[log['y'], log['x']])
    # nothing allowed: no component whatever the threshold
    op2, twin2, q = make_op(G, P, [0, 4, 9], border, 0.1, dirty, psf, mask=np.zeros((G, G), bool))
    assert len(_run_both(op2, twin2, q, patch, 0.0, 10)) == 0


@gpu
def test_cycles_ties():
    """Integer-valued image and PSF, scales [0]: equal peaks within a tile and across tiles go to
    the first in row-major order."""
    G, P, border, patch = 96, 1, 0.02, (1, 9, 9)
    rng = np.random.default_rng(24)
    dirty = rng.integers(-6, 7, (P, G, G)).astype(np.float32)
    dirty[0, 10, 50] = dirty[0, 10, 51] = dirty[0, 70, 12] = dirty[0, 12, 80] = 16   # tied peaks
    dirty[0, 40, 40] = -16
    psf = (rng.integers(-1, 2, (P, G, G)) * 0.25).astype(np.float32)
    psf[:, G // 2, G // 2] = 1
    op, twin, q = make_op(G, P, [0], border, 0.5, dirty, psf)
    log = _run_both(op, twin, q, patch, 0.0)
    assert (log['y'][0], log['x'][0]) == (10, 50)
    values, counts = np.unique(log['peak'], return_counts=True)
    assert counts.max() > 3                                         # ties did occur


@gpu
def test_cycles_six_scales_boxes_larger_than_image():
    G, P, border, patch = 160, 1, 0.02, (1, 15, 17)
    dirty, psf = field(G, P, border, 25)
    scales = [0, 4, 9, 18, 30, 50]
    op, twin, q = make_op(G, P, scales, border, 0.1, dirty, psf)
    assert twin.params.radii[-1] == 64
    op.reset()
    op.prepare(patch)
    twin.prepare(patch)
    n, inv = op.scale_norms()
    np.testing.assert_array_equal(n, twin.norms)
    np.testing.assert_array_equal(inv, twin.inv)
    for j, k in [(5, 5), (2, 5), (5, 3), (4, 4)]:          # cross radii 128, 76, 87, 78
        X = op.cross_patch(j, k)
        assert X.shape == twin.cross[j, k].shape
        np.testing.assert_array_equal(X, twin.cross[j, k], 'X %d %d' % (j, k))
    assert op.cross_patch(5, 5).shape == (1, G, G)          # larger than the image: clipped to it
    log = _run_both(op, twin, q, patch, 0.0)
    assert len(log) == CYCLES


@gpu
@pytest.mark.parametrize('name', ['i', 'clipped', 'threshold'])
def test_single_scale_is_the_existing_path(name):
    """scales = [0] on the device against kimg_clean_cycles on the same data: the same components,
    residual, model and tile records, exactly."""
    from katsdpimager_amd import clean, parameters
    c = gi.CLEAN_CONFIGS[name]
    ci = gi.clean_inputs(c)
    G, P = c['pixels'], c['P']
    op, twin, q = make_op(G, P, [0], c['border'], c['loop_gain'], ci['dirty'], ci['psf'])
    op.reset()
    log = op.run_cycles(ci['psf_patch'], c['threshold'], c['cycles'])
    ctx, q = context_queue()
    ip, cp = _params(G, P, c['border'], c['loop_gain'])
    fn = clean.CleanTemplate(ctx, cp, np.float32, P).instantiate(q, ip)
    fn.ensure_all_bound()
    fn.buffer('dirty').set(q, ci['dirty'])
    fn.buffer('psf').set(q, ci['psf'])
    fn.buffer('model').zero(q)
    fn.reset()
    fn.run_cycles(ci['psf_patch'], c['threshold'], c['cycles'], collect=False)
    values, pos, pix = fn._collect_cycle_arrays()
    assert len(log) == len(values) > 10
    assert np.all(log['scale'] == 0)
    np.testing.assert_array_equal(log['peak'], values)
    np.testing.assert_array_equal(np.stack([log['y'], log['x']], axis=1), pos)
    np.testing.assert_array_equal(log['flux'], pix)
    np.testing.assert_array_equal(op.buffer('dirty').get(q), fn.buffer('dirty').get(q))
    np.testing.assert_array_equal(op.buffer('model').get(q), fn.buffer('model').get(q))
    tmax, tpos = op.tile_records()
    np.testing.assert_array_equal(tmax[0], fn.buffer('tile_max').get(q))
    np.testing.assert_array_equal(tpos[0], fn.buffer('tile_pos').get(q))


@gpu
def test_single_scale_is_the_existing_path_four_polarizations():
    """gi.CLEAN_CONFIGS has no problem with four polarizations in mode CLEAN_I, so this one is made
    here: field(96, 4, ...) with scales = [0] against kimg_clean_cycles on the same data, exactly as
    above; the four fluxes of every component included."""
    from katsdpimager_amd import clean
    G, P, border, loop_gain, patch, cycles = 96, 4, 0.02, 0.1, (4, 15, 17), 150
    dirty, psf = field(G, P, border, 26)
    op, twin, q = make_op(G, P, [0], border, loop_gain, dirty, psf)
    op.reset()
    log = op.run_cycles(patch, 0.0, cycles)
    ctx, q = context_queue()
    ip, cp = _params(G, P, border, loop_gain)
    fn = clean.CleanTemplate(ctx, cp, np.float32, P).instantiate(q, ip)
    fn.ensure_all_bound()
    fn.buffer('dirty').set(q, dirty)
    fn.buffer('psf').set(q, psf)
    fn.buffer('model').zero(q)
    fn.reset()
    fn.run_cycles(patch, 0.0, cycles, collect=False)
    values, pos, pix = fn._collect_cycle_arrays()
    assert len(log) == len(values) == cycles
    assert np.all(log['scale'] == 0)
    np.testing.assert_array_equal(log['peak'], values)
    np.testing.assert_array_equal(np.stack([log['y'], log['x']], axis=1), pos)
    assert pix.shape == (cycles, P)
    np.testing.assert_array_equal(log['flux'], pix)
    np.testing.assert_array_equal(op.buffer('dirty').get(q), fn.buffer('dirty').get(q))
    np.testing.assert_array_equal(op.buffer('model').get(q), fn.buffer('model').get(q))
    tmax, tpos = op.tile_records()
    np.testing.assert_array_equal(tmax[0], fn.buffer('tile_max').get(q))
    np.testing.assert_array_equal(tpos[0], fn.buffer('tile_pos').get(q))
    same_log(log, twin.run_cycles(patch, 0.0, cycles))


# ---- the imager and the driver -------------------------------------------------------------------------

def _channel(c):
    from helpers import make_params
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
def test_imager_reset_repeats_the_log():
    """Imaging.multiscale_reset after a first run, on the buffers put back: the same log again."""
    from katsdpimager_amd import imaging
    c = gi.E2E_CONFIGS['degrid']
    ctx, q, ip, gp, ap, wp, cp, reader = _channel(c)
    im = imaging.ImagingTemplate(ctx, ap, ip.fixed, wp, gp.fixed, cp).instantiate(
        q, ip, gp, c['vis_block'], 0, 2)
    im.ensure_all_bound()
    G, P = c['pixels'], c['P']
    dirty, psf = field(G, P, c['border'], 31)
    patch = (P, 15, 17)
    with pytest.raises(ValueError):
        im.multiscale_reset()
    im.set_multiscale(ms.MultiScaleParameters([0, 4, 9]))
    logs = []
    for _ in range(2):
        im.set_buffer('dirty', dirty)
        im.set_buffer('psf', psf)
        im.clear_model()
        im.multiscale_reset()
        logs.append(im.multiscale_cycles(patch, 0.0, 70))
    assert len(logs[0]) == 70
    same_log(logs[1], logs[0])
    twin = ms.MultiScaleCleanHost(ms.MultiScaleParameters([0, 4, 9]), c['border'], c['loop_gain'],
                                  CLEAN_I, dirty.copy(), psf, np.zeros_like(dirty))
    same_log(logs[0], twin.run_cycles(patch, 0.0, 70))
    np.testing.assert_array_equal(im.get_buffer('model'), twin.model)


@gpu
def test_driver_end_to_end():
    """process_channel(multiscale=...) on the synthetic channel of the end-to-end tests: two major
    cycles, the second one's first peak below the first one's; the refusals; and the default path
    before and after gives the same result (to the run-to-run bounds of two runs of one driver,
    whose gridders' float atomics differ in the last bits: tests/test_clean_mask.py)."""
    from katsdpimager_amd import clean, frontend, imaging
    c = gi.E2E_CONFIGS['degrid']
    assert c['mode'] == CLEAN_I and c['degrid']
    ctx, q, ip, gp, ap, wp, cp, reader = _channel(c)

    def drive(**kwargs):
        im = imaging.ImagingTemplate(ctx, ap, ip.fixed, wp, gp.fixed, cp).instantiate(
            q, ip, gp, c['vis_block'], 0, 2)
        im.ensure_all_bound()
        kwargs.setdefault('degrid', True)
        degrid = kwargs.pop('degrid')
        stats = frontend.process_channel(reader, 0, im, ip, gp, cp, wp.weight_type, c['vis_block'],
                                         2, degrid, **kwargs)
        return stats, im.get_buffer('dirty'), im.get_buffer('model')

    before, d0, m0 = drive()
    params = ms.MultiScaleParameters([0, 4, 9])
    stats, d1, m1 = drive(multiscale=params)
    assert stats['major'] == 2 and len(stats['peaks']) == 2 and stats['minor'] > 0
    assert stats['peaks'][1] < stats['peaks'][0]
    assert np.any(m1 != 0) and np.all(np.isfinite(d1))
    with pytest.raises(ValueError):
        drive(multiscale=params, degrid=False)
    with pytest.raises(ValueError):
        drive(multiscale=params, clean_batcher=clean.CleanBatcher(1))
    after, d2, m2 = drive()
    assert set(before) == set(after)
    for key in ('major', 'minor', 'psf_patch'):
        assert before[key] == after[key], key
    for key in ('weights_noise', 'normalized_noise', 'noise', 'scale'):
        np.testing.assert_allclose(after[key], before[key], rtol=1e-4, err_msg=key)
    np.testing.assert_allclose(after['peaks'], before['peaks'], rtol=1e-4)
    assert np.max(np.abs(m2 - m0)) <= 1e-5 * np.max(np.abs(m0))
