"""kimg_primary_beam on the device against its numpy statement (primary_beam.sample_host,
correct_host), bit for bit: every polarization count, dense and padded layouts (16-byte rows and
the element-by-element route), the smallest and largest tables, the exact ends of the table, a
threshold that equals a pixel's power, an all-NaN row, the two partial forms (sample only, images
only), the two-pass route through kimg_apply_primary_beam, and the operator, the imager's method
and the driver's keyword on the small end-to-end channel."""
import numpy as np
import pytest

from helpers import Padded, context_queue
import golden_inputs as gi
from katsdpimager_amd import primary_beam as pb
from katsdpimager_amd.primary_beam import RadialBeam, PrimaryBeamParameters

pytestmark = pytest.mark.gpu

PIXEL = 0.001
# (W, H): one 16-byte chunk per lane and several rows per workgroup; a width that is no multiple of
# 4; the smallest; more than one workgroup along a row; more rows than the 2048 workgroups of a
# launch take at once (a column of workgroups walks down the image from 8192 rows)
SHAPES = [(64, 64), (70, 6), (5, 3), (300, 5), (8, 8200)]
# rows on 16-byte boundaries (dense, and padded to a pitch that is a multiple of 4: 72 for width 70,
# the tail of a row element by element) and the route without them (an odd pitch, the pointer one
# element off)
LAYOUTS = ['dense', 'padded16', 'odd']


def layout_args(layout, W):
    if layout == 'padded16':
        return dict(rpad=(-W) % 4 + 4, vpad=1, origin=(1, 0))
    if layout == 'odd':
        return dict(rpad=4 + W % 2, vpad=2, origin=(3, 1))
    return dict()


def L():
    from katsdpimager_amd import _lib
    return _lib.lib()


def device_row(ctx, q, row):
    from katsdpimager_amd import accel
    d = accel.DeviceArray(ctx, row.shape, np.float32)
    d.set(q, row)
    return d


def geometry(W, H):
    """Pixels PIXEL apart, the centre of the beam half the shorter side from the first pixel (the
    imager's bias on a square image; one bias serves both axes)."""
    return PIXEL, -0.5 * min(W, H) * PIXEL


def beam_row(W, H, R, fraction=0.8):
    """A cosine-taper row of R samples that ends at `fraction` of the largest radius of the grid, so
    that the far pixels are NaN, with its half-power point at a third of that radius."""
    scale, bias = geometry(W, H)
    far = np.hypot(max(abs(bias), abs((W - 1) * scale + bias)),
                   max(abs(bias), abs((H - 1) * scale + bias)))
    reach = fraction * far
    step = reach / (R - 1)
    beam = RadialBeam.cosine_taper(2.0 * reach / 3.0, 1.0e9, [1.0e9], step, reach)
    row = beam.row(1.0e9)[:R]
    assert len(row) == R
    return row, step


def images(P, H, W, seed):
    rs = np.random.RandomState(seed)
    model = rs.standard_normal((P, H, W)).astype(np.float32)
    model[rs.uniform(size=model.shape) < 0.5] = 0.0
    dirty = rs.standard_normal((P, H, W)).astype(np.float32)
    return model, dirty


def run(ctx, q, row, step, W, H, P, threshold, layout, model=None, dirty=None, beam=True,
        scale_bias=None):
    """One call on padded copies; returns (beam_power, model, dirty) as far as they were given, the
    padding of each checked."""
    scale, bias = scale_bias or geometry(W, H)
    d_row = device_row(ctx, q, row)
    kw = layout_args(layout, W)
    if layout != 'dense':
        pitch = kw['origin'][1] + W + kw['rpad']
        assert pitch % 4 == 0 if layout == 'padded16' else pitch % 2 == 1
    d_beam = Padded(ctx, q, np.full((H, W), 7.0, np.float32), **kw) if beam else None
    d_model = Padded(ctx, q, model, **kw) if model is not None else None
    d_dirty = Padded(ctx, q, dirty, **kw) if dirty is not None else None
    pitched = d_model or d_beam
    rc = L().kimg_primary_beam(
        d_beam.ptr if beam else None, d_beam.row if beam else 0,
        d_model.ptr if d_model else None, d_dirty.ptr if d_dirty else None, pitched.row, pitched.pol,
        W, H, P, d_row.ptr, len(row), float(pb.inv_step32(step)), scale, bias, threshold, q.handle)
    assert rc == 0
    return (d_beam.get(q) if beam else None, d_model.get(q) if d_model else None,
            d_dirty.get(q) if d_dirty else None)


def expect(row, step, W, H, threshold, model, dirty, scale_bias=None):
    scale, bias = scale_bias or geometry(W, H)
    power = pb.sample_host(row, step, W, H, scale, bias)
    model, dirty = model.copy(), dirty.copy()
    keep = pb.correct_host(power, model, dirty, threshold)
    return power, model, dirty, keep


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('P', [1, 2, 3, 4])
@pytest.mark.parametrize('W,H', SHAPES)
def test_fused_pass_is_the_host_contract(W, H, P, layout):
    ctx, q = context_queue()
    row, step = beam_row(W, H, 257)
    model, dirty = images(P, H, W, W + P)
    want_power, want_model, want_dirty, keep = expect(row, step, W, H, 0.1, model, dirty)
    assert np.isnan(want_power).any() and keep.any() and (~keep & ~np.isnan(want_power)).any()
    power, got_model, got_dirty = run(ctx, q, row, step, W, H, P, 0.1, layout, model, dirty)
    np.testing.assert_array_equal(power, want_power)
    np.testing.assert_array_equal(got_model, want_model)
    np.testing.assert_array_equal(got_dirty, want_dirty)
    assert not np.isnan(got_model).any()


@pytest.mark.parametrize('R', [2, 257, 4096])
def test_table_sizes(R):
    """The smallest table (one interval: nearly every pixel NaN), an ordinary one and the largest
    the entry point takes."""
    from katsdpimager_amd import _lib
    assert _lib.PRIMARY_BEAM_MAX_SAMPLES == 4096
    ctx, q = context_queue()
    W, H, P = 70, 66, 2
    if R == 2:
        row, step = np.array([1.0, 0.25], np.float32), 2.5 * PIXEL
    else:
        row, step = beam_row(W, H, R)
    model, dirty = images(P, H, W, R)
    want_power, want_model, want_dirty, keep = expect(row, step, W, H, 0.3, model, dirty)
    assert keep.any() and np.isnan(want_power).any()
    if R == 2:
        assert np.isnan(want_power).mean() > 0.95
    for layout in ('dense', 'odd'):
        power, got_model, got_dirty = run(ctx, q, row, step, W, H, P, 0.3, layout, model, dirty)
        np.testing.assert_array_equal(power, want_power)
        np.testing.assert_array_equal(got_model, want_model)
        np.testing.assert_array_equal(got_dirty, want_dirty)


def test_exact_ends_of_the_table():
    """l, m = -2 .. 2 in whole steps: s = 0 at the centre (the first sample), s = 1 one pixel off
    (the second sample itself), s = R - 1 = 2 two pixels off: NaN, as everything beyond."""
    ctx, q = context_queue()
    row = np.array([0.75, -0.5, 0.25], np.float32)
    geometry_ = (1.0, -2.0)
    power, _, _ = run(ctx, q, row, 1.0, 5, 5, 1, 0.0, 'dense', scale_bias=geometry_)
    np.testing.assert_array_equal(power, pb.sample_host(row, 1.0, 5, 5, *geometry_))
    assert power[2, 2] == np.float32(0.75) ** 2
    assert power[2, 3] == power[1, 2] == np.float32(0.25)
    assert np.isnan(power[2, 4]) and np.isnan(power[0, 2]) and np.isnan(power[0, 0])
    assert not np.isnan(power[1, 1])            # s = sqrt(2): inside the second interval
    assert np.isnan(power).sum() == 25 - 9


def test_threshold_equal_to_a_power_keeps_the_pixel():
    ctx, q = context_queue()
    W, H, P = 70, 6, 3
    row, step = beam_row(W, H, 257)
    model, dirty = images(P, H, W, 9)
    power = pb.sample_host(row, step, W, H, *geometry(W, H))
    y, x = 2, 17
    threshold = float(power[y, x])
    assert 0.0 < threshold < 1.0
    want_power, want_model, want_dirty, keep = expect(row, step, W, H, threshold, model, dirty)
    assert keep[y, x] and 0 < keep.sum() < keep.size
    for layout in LAYOUTS:
        _, got_model, got_dirty = run(ctx, q, row, step, W, H, P, threshold, layout, model, dirty)
        np.testing.assert_array_equal(got_model, want_model)
        np.testing.assert_array_equal(got_dirty, want_dirty)
        assert not np.isnan(got_dirty[:, y, x]).any()


def test_all_nan_row_blanks_everything():
    """A frequency outside the model's range: model 0, dirty NaN, beam NaN."""
    ctx, q = context_queue()
    W, H, P = 64, 64, 2
    beam = RadialBeam.cosine_taper(0.05, 1.0e9, [0.9e9, 1.1e9], 0.001, 0.1)
    row = beam.row(1.2e9)
    assert np.all(np.isnan(row))
    model, dirty = images(P, H, W, 4)
    power, got_model, got_dirty = run(ctx, q, row, beam.step, W, H, P, 0.1, 'dense', model, dirty)
    assert np.all(np.isnan(power)) and np.all(np.isnan(got_dirty))
    assert not np.any(got_model) and not np.isnan(got_model).any()


@pytest.mark.parametrize('layout', ['dense', 'odd'])
def test_partial_forms(layout):
    """Sample only (the images NULL) writes the beam and nothing around it; images only (the beam
    NULL) corrects as the full pass does."""
    ctx, q = context_queue()
    W, H, P = 70, 6, 2
    row, step = beam_row(W, H, 257)
    model, dirty = images(P, H, W, 5)
    want_power, want_model, want_dirty, _ = expect(row, step, W, H, 0.1, model, dirty)
    power, none_m, none_d = run(ctx, q, row, step, W, H, P, 0.1, layout)     # (.get checks the guards)
    assert none_m is None and none_d is None
    np.testing.assert_array_equal(power, want_power)
    none_p, got_model, got_dirty = run(ctx, q, row, step, W, H, P, 0.1, layout, model, dirty, beam=False)
    assert none_p is None
    np.testing.assert_array_equal(got_model, want_model)
    np.testing.assert_array_equal(got_dirty, want_dirty)


@pytest.mark.parametrize('P', [1, 4])
def test_fused_pass_is_sample_then_the_two_applies(P):
    """... wherever the beam is not NaN (there the apply kernel leaves NaN in the model)."""
    ctx, q = context_queue()
    W, H = 70, 66
    row, step = beam_row(W, H, 257)
    model, dirty = images(P, H, W, 6)
    _, fused_model, fused_dirty = run(ctx, q, row, step, W, H, P, 0.1, 'dense', model, dirty)
    power, _, _ = run(ctx, q, row, step, W, H, P, 0.1, 'dense')
    d_beam = Padded(ctx, q, power)
    outs = []
    for image, replacement in ((model, 0.0), (dirty, float('nan'))):
        d = Padded(ctx, q, image)
        assert L().kimg_apply_primary_beam(d.ptr, d.row, d.pol, d_beam.ptr, d_beam.row, W, H, P, 0.1,
                                           replacement, q.handle) == 0
        outs.append(d.get(q))
    finite = ~np.isnan(power)
    assert finite.any() and not finite.all()
    np.testing.assert_array_equal(fused_model[:, finite], outs[0][:, finite])
    np.testing.assert_array_equal(fused_dirty[:, finite], outs[1][:, finite])
    assert np.all(np.isnan(outs[0][:, ~finite])) and not np.any(fused_model[:, ~finite])


def test_operator():
    """PrimaryBeamTemplate / PrimaryBeam: slots, attributes, sample() and the fused call."""
    from katsdpimager_amd import accel
    ctx, q = context_queue()
    W = H = 64
    P = 2
    with pytest.raises(ValueError):
        pb.PrimaryBeamTemplate(ctx, np.float64, P)
    op = pb.PrimaryBeamTemplate(ctx, np.float32, P).instantiate(q, (P, H, W))
    assert isinstance(op, accel.Operation) and set(op.slots) == {'beam_power', 'model', 'dirty'}
    with pytest.raises(RuntimeError):
        op()
    row, step = beam_row(W, H, 129)
    op.set_model_row(row, step)
    op.lm_scale, op.lm_bias = geometry(W, H)
    op.threshold = 0.2
    assert op.row.shape == (129,) and op.step == step
    np.testing.assert_array_equal(op.row.get(q), row)
    op.sample()
    want_power = pb.sample_host(row, step, W, H, *geometry(W, H))
    np.testing.assert_array_equal(op.buffer('beam_power').get(q), want_power)
    model, dirty = images(P, H, W, 8)
    op.ensure_all_bound()
    op.buffer('model').set(q, model)
    op.buffer('dirty').set(q, dirty)
    op.buffer('beam_power').zero(q)
    op()
    _, want_model, want_dirty, _ = expect(row, step, W, H, 0.2, model, dirty)
    np.testing.assert_array_equal(op.buffer('beam_power').get(q), want_power)
    np.testing.assert_array_equal(op.buffer('model').get(q), want_model)
    np.testing.assert_array_equal(op.buffer('dirty').get(q), want_dirty)


def find_peak_numpy(image, pbeam, noise):
    """frontend.find_peak: the largest |pixel| among those with |pixel| * pbeam > 7.5 * noise, in
    the kernel's float32; NaN when there is none."""
    limit = np.float32(7.5) * np.float32(noise)
    v = np.abs(image)
    with np.errstate(invalid='ignore'):
        passes = (v * pbeam[np.newaxis]) > limit
    return float(v[passes].max()) if passes.any() else float('nan')


def test_imager_and_driver():
    """The small end-to-end channel.  Imaging.primary_beam_correct after a plain run: the beam is
    sample_host, model and dirty are correct_host of what the run left, exactly.
    process_channel(primary_beam=...) on a fresh imager: the result's keys; the same beam; model and
    dirty are correct_host of the images as they stood when the driver made its call (caught on
    the way in), exactly; and those images are the plain run's to the bounds two runs of one driver
    keep (tests/test_clean_mask.py: the gridders' float atomics differ in the last bits from run to
    run, which is why the comparison across runs cannot be exact).  find_peak with the returned
    beam is its numpy restatement."""
    import test_clean_mask as tcm
    from helpers import kernel_taper, relerr, tapered_relerr
    from katsdpimager_amd import frontend, imaging
    c = gi.E2E_CONFIGS['degrid']
    ctx, q, ip, gp, ap, wp, cp, reader = tcm._channel(c)
    G = c['pixels']
    frequency = pb.SPEED_OF_LIGHT / ip.wavelength
    beam = RadialBeam.cosine_taper(0.06, 1.5e9, [1.4e9, 1.6e9], 2.5e-4, 0.06)
    assert beam.frequencies[0] < frequency < beam.frequencies[1]
    params = PrimaryBeamParameters(beam, cutoff=0.1)
    lm_scale, lm_bias = float(ip.pixel_size), -0.5 * G * float(ip.pixel_size)
    want_power = pb.sample_host(beam.row(frequency), beam.step, G, G, lm_scale, lm_bias)
    assert np.isnan(want_power).any() and (want_power < 0.1).any() and (want_power > 0.9).any()

    def drive(**kwargs):
        im = imaging.ImagingTemplate(ctx, ap, ip.fixed, wp, gp.fixed, cp).instantiate(
            q, ip, gp, c['vis_block'], 0, c['major'])
        im.ensure_all_bound()
        stats = frontend.process_channel(reader, 0, im, ip, gp, cp, wp.weight_type, c['vis_block'],
                                         c['major'], c['degrid'], **kwargs)
        return im, stats

    im0, plain = drive()
    assert not {'primary_beam', 'beam_power', 'beam_valid'} & set(plain)
    model0, dirty0 = im0.get_buffer('model'), im0.get_buffer('dirty')
    assert np.any(model0)
    returned = im0.primary_beam_correct(params, frequency)
    assert returned is im0.buffer('beam_power')
    np.testing.assert_array_equal(returned.get(q), want_power)
    want_model, want_dirty = model0.copy(), dirty0.copy()
    keep = pb.correct_host(want_power, want_model, want_dirty, 0.1)
    np.testing.assert_array_equal(im0.get_buffer('model'), want_model)
    np.testing.assert_array_equal(im0.get_buffer('dirty'), want_dirty)
    assert im0.beam_valid(0.1) == int(keep.sum())
    assert im0.beam_valid(0.0) == int((~np.isnan(want_power)).sum())

    caught = {}
    correct = imaging.Imaging.primary_beam_correct

    def catching(self, *args):
        caught['model'], caught['dirty'] = self.get_buffer('model'), self.get_buffer('dirty')
        caught['args'] = args
        return correct(self, *args)
    imaging.Imaging.primary_beam_correct = catching
    try:
        im1, stats = drive(primary_beam=params)
    finally:
        imaging.Imaging.primary_beam_correct = correct
    assert stats['primary_beam'] is params and caught['args'] == (params, frequency)
    assert stats['beam_power'] is im1.buffer('beam_power')
    assert stats['beam_valid'] == int(keep.sum())
    assert stats['major'] == plain['major'] and stats['minor'] == plain['minor']
    np.testing.assert_array_equal(stats['beam_power'].get(q), want_power)
    want_model, want_dirty = caught['model'].copy(), caught['dirty'].copy()
    pb.correct_host(want_power, want_model, want_dirty, 0.1)
    got_model, got_dirty = im1.get_buffer('model'), im1.get_buffer('dirty')
    np.testing.assert_array_equal(got_model, want_model)
    np.testing.assert_array_equal(got_dirty, want_dirty)
    taper = kernel_taper(c)
    inner = np.s_[:, G // 8:-G // 8, G // 8:-G // 8]
    assert tapered_relerr(caught['dirty'], dirty0, taper) < 1e-5
    assert relerr(caught['dirty'][inner], dirty0[inner]) < 1e-4
    assert relerr(caught['model'], model0) < 1e-5

    for noise in (float(stats['noise']), 0.01 * float(stats['noise'])):
        for name, image in (('dirty', got_dirty), ('model', got_model)):
            got = frontend.find_peak(q, im1.buffer(name), stats['beam_power'], noise)
            want = find_peak_numpy(image, want_power, noise)
            assert got == want or (got != got and want != want), (name, noise, got, want)
    assert want == want         # (at a hundredth of the noise something passes)
