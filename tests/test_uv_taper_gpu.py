"""The uv taper on the device: kimg_density_weights_taper through the C ABI on sentinel-padded
layouts against the untapered entry points and weight.uv_taper_host, then through the operators
(Weights, Imaging, frontend.process_channels).

Bounds.  With d the device's own untapered float32 result and T the float64 twin, the kernel stores
fl(d * fl(T')) where T' is its own float64 evaluation of T (a few 1e-16 from numpy's): one rounding
of t and one of the product, (1 + e1)(1 + e2) with |e| <= 2^-24, i.e. 2 * 2^-24 plus second-order
terms and the 1e-16 -- asserted as 3 * 2^-24 |d T|.  That holds where fl(T) is a normal float32;
below the smallest normal (2^-126) roundings are absolute, 2^-150 each, and the bound is 2^-126
absolute.  The weights of these tests are at least 1, so that d <= 1 under all three weightings and
d T is below 2^-126 wherever T is: a subnormal t times a d above 1 could come out normal with the
subnormal's coarser relative rounding, which neither bound describes (include/kimg.h says so).

Sums: n non-negative terms added in any order in float64 carry at most n * 2^-53 relative error
(one rounding per addition, and one for the product e * (e w); e * w is exact in float64); the
host's sums are taken in extended precision from the device's own output grid."""
import ctypes
import math

import numpy as np
import pytest

from helpers import Padded, context_queue, make_params, relerr, tapered_relerr, kernel_taper
import golden_inputs as gi
from katsdpimager_amd.weight import UVTaperParameters, WeightType, uv_taper_host

pytestmark = pytest.mark.gpu
KIMG_EINVAL = -10001
EPS32 = 2.0 ** -24
TINY32 = 2.0 ** -126
IMAGE_SIZE = 0.02           # cells 50 wavelengths apart

SHAPES = [(2, 2), (6, 10), (254, 4), (258, 6), (64, 64), (2, 4100), (520, 1030)]      # (W, H)
shapes = pytest.mark.parametrize('W,H', SHAPES)
pols = pytest.mark.parametrize('P', [1, 2, 3, 4])
ROBUST = (5 * 10 ** -0.5) ** 2


def L():
    from katsdpimager_amd import _lib
    return _lib.lib()


def taper_struct(params):
    from katsdpimager_amd import _lib
    return _lib.UVTaper(*params.coefficients())


def make_weights(W, H, P, seed):
    """Random weights in [1, 4) with about a third of the cells exactly 0."""
    rs = np.random.RandomState(seed)
    w = rs.uniform(1.0, 4.0, (P, H, W)).astype(np.float32)
    w[rs.uniform(size=w.shape) < 1.0 / 3.0] = 0.0
    return w


def padded(ctx, q, array):
    return Padded(ctx, q, array, rpad=5, vpad=2, origin=(1, 3))


def sums_buffer(ctx, q):
    return Padded(ctx, q, np.full((1, 3), 3.0), rpad=2, vpad=1, origin=(1, 1))


def run(ctx, q, weights, kind, params=None):
    """One density pass over a padded copy of ``weights``: kind 'natural' (a = 0, b = 1), 'uniform'
    (a = 1, b = 0) or 'robust' (mean weight on the device, b = 1); ``params`` None = the untapered
    entry points.  Returns (grid, sums); the padding of both has been checked."""
    P, H, W = weights.shape
    g = padded(ctx, q, weights)
    sums = sums_buffer(ctx, q)
    mean_sums = None
    if kind == 'robust':
        mean_sums = sums_buffer(ctx, q)
        assert L().kimg_mean_weight(mean_sums.ptr, g.ptr, g.row, W, H, q.handle) == 0
    a, b = {'natural': (0.0, 1.0), 'uniform': (1.0, 0.0), 'robust': (0.0, 1.0)}[kind]
    args = (sums.ptr, g.ptr, g.row, g.pol, W, H, P)
    if params is None:
        if kind == 'robust':
            rc = L().kimg_density_weights_robust(*args, mean_sums.ptr, ROBUST, b, q.handle)
        else:
            rc = L().kimg_density_weights(*args, a, b, q.handle)
    else:
        t = taper_struct(params)
        step = 1.0 / IMAGE_SIZE
        rc = L().kimg_density_weights_taper(
            *args, a, b, mean_sums.ptr if mean_sums is not None else None,
            ROBUST if mean_sums is not None else 0.0, step, step, ctypes.byref(t), q.handle)
    assert rc == 0
    return g.get(q), sums.get(q)[0]


def busy_taper(W, H):
    """An elliptical Gaussian at 30 degrees, both cuts and both ramps, scaled to the grid: the
    exponent reaches 500 along the major axis at the corner radius R (float32 underflows from 104,
    float64 only from 745), the cuts stand at 0.013 R and 0.83 R with ramps of 0.021 R and 0.2 R."""
    R = math.hypot(W / 2, H / 2) / IMAGE_SIZE
    major = math.sqrt(500.0 / (math.pi ** 2 / (4 * math.log(2)))) / R
    return UVTaperParameters((major, 0.5 * major, math.radians(30.0)), min_uv=0.013 * R,
                             max_uv=0.83 * R, inner_tukey=0.021 * R, outer_tukey=0.2 * R), R


def check_values(out, d_dev, T, weights):
    want = d_dev.astype(np.float64) * T
    bound = np.where(want >= TINY32, 3 * EPS32 * want, TINY32)
    err = np.abs(out.astype(np.float64) - want)
    assert np.all(err <= bound), (float((err / bound).max()), np.unravel_index(np.argmax(err / bound), err.shape))
    zero = (np.broadcast_to(T, out.shape) == 0) | (weights == 0)
    assert np.all(out[zero] == 0)
    assert not np.any(np.signbit(out))


def host_sums(out, weights, T):
    """(sums, bound) from the device's output grid, polarization 0."""
    e = out[0].astype(np.longdouble).ravel()
    w = weights[0].astype(np.longdouble).ravel()
    counted = (T > 0).ravel()
    sums = np.array([float(w[counted].sum()), float((e * w).sum()), float((e * e * w).sum())])
    return sums, e.size * 2.0 ** -53 * sums


@shapes
@pols
def test_identity_taper_is_the_plain_pass(W, H, P):
    """No Gaussian, no cuts: t = 1, and the grid is kimg_density_weights' / _robust's bit for bit
    under natural, uniform and robust weighting; the sums agree within n * 2^-53 relative."""
    ctx, q = context_queue()
    weights = make_weights(W, H, P, 100 + W + H + P)
    n = W * H
    for kind in ('natural', 'uniform', 'robust'):
        plain, plain_sums = run(ctx, q, weights, kind)
        got, got_sums = run(ctx, q, weights, kind, UVTaperParameters())
        np.testing.assert_array_equal(got.view(np.uint32), plain.view(np.uint32))
        assert np.all(np.abs(got_sums - plain_sums) <= n * 2.0 ** -53 * plain_sums), (kind, got_sums, plain_sums)
        assert np.all(got[weights == 0] == 0)


@shapes
@pols
def test_values_and_sums(W, H, P):
    """Gaussian, cuts and ramps together: every cell within 3 * 2^-24 of d_dev * T (2^-126 absolute
    below the smallest normal), exact zeros where T == 0 or W == 0, the sums within n * 2^-53 of the
    host's sums over the device's own grid, sums[0] without exactly the cells with T == 0.  (The
    module docstring derives the bounds.)"""
    ctx, q = context_queue()
    weights = make_weights(W, H, P, 200 + W + H + P)
    params, R = busy_taper(W, H)
    T = uv_taper_host((H, W), IMAGE_SIZE, params)
    # the cuts fall between cells, and the taper does what the test is about
    step = 1.0 / IMAGE_SIZE
    r = np.hypot(*np.meshgrid((np.arange(W) - W // 2) * step, (np.arange(H) - H // 2) * step))
    for radius in (params.min_uv, params.max_uv, params.min_uv + params.inner_tukey,
                   params.max_uv - params.outer_tukey):
        assert np.all(np.abs(r - radius) > 1e-9 * R)
    if W * H >= 1000:
        assert np.any(T == 0) and np.any((T > 0) & (T < 2.0 ** -150)) and np.any(T > 0.5)
        assert np.any((T >= 2.0 ** -149) & (T < TINY32))
        assert np.any((T == 0) & (weights[0] != 0))
    n = W * H
    for kind in ('natural', 'uniform', 'robust'):
        d_dev, _ = run(ctx, q, weights, kind)
        out, sums = run(ctx, q, weights, kind, params)
        check_values(out, d_dev, T, weights)
        want, bound = host_sums(out, weights, T)
        assert np.all(np.abs(sums - want) <= bound), (kind, sums, want, bound)
        if W * H >= 1000:
            # the count is a different number with the cut cells in it
            assert float(weights[0].astype(np.float64).sum()) - want[0] > 4 * bound[0]


def test_rejected_arguments_write_nothing():
    ctx, q = context_queue()
    W, H, P = 6, 10, 2
    weights = make_weights(W, H, P, 7)
    g = padded(ctx, q, weights)
    sums = sums_buffer(ctx, q)
    step = 1.0 / IMAGE_SIZE
    good = UVTaperParameters((2e-3, 1e-3, 0.5), 10.0, 400.0, 20.0, 50.0).coefficients()
    from katsdpimager_amd import _lib

    def call(taper=good, sums_ptr=sums.ptr, grid_ptr=g.ptr, row=g.row, width=W, height=H,
             steps=(step, step), null_taper=False):
        t = _lib.UVTaper(*taper)
        return L().kimg_density_weights_taper(
            sums_ptr, grid_ptr, row, g.pol, width, height, P, 1.0, 0.0, None, 0.0, steps[0],
            steps[1], None if null_taper else ctypes.byref(t), q.handle)

    assert call(null_taper=True) == KIMG_EINVAL
    assert call(sums_ptr=None) == KIMG_EINVAL
    assert call(grid_ptr=None) == KIMG_EINVAL
    for field in range(7):
        for bad in (float('nan'), float('inf'), -float('inf')):
            fields = list(good)
            fields[field] = bad
            assert call(taper=tuple(fields)) == KIMG_EINVAL, (field, bad)
    for field in (0, 2, 3, 4, 5, 6):
        fields = list(good)
        fields[field] = -1.0
        assert call(taper=tuple(fields)) == KIMG_EINVAL, field
    assert call(steps=(float('nan'), step)) == KIMG_EINVAL
    assert call(steps=(step, 0.0)) == KIMG_EINVAL
    assert call(row=W - 1) == KIMG_EINVAL
    assert call(width=W - 1) == KIMG_EINVAL         # odd
    assert call(height=H - 1) == KIMG_EINVAL        # odd
    np.testing.assert_array_equal(g.get(q), weights)
    np.testing.assert_array_equal(sums.get(q)[0], np.full(3, 3.0))
    assert call() == 0
    assert not np.array_equal(g.get(q), weights)


# ---------------------------------------------------------------------------------------------
# through the operators

def _imager(c, weight_type, taper, queue=None):
    from katsdpimager_amd import imaging, parameters
    ctx, q = context_queue()
    q = queue or q
    ip, gp, ap = make_params(c)
    wp = parameters.WeightParameters(weight_type, c['robustness'], taper)
    cp = parameters.CleanParameters(c['minor'], c['loop_gain'], c['major_gain'], c['threshold'],
                                    c['mode'], c['psf_cutoff'], c['psf_limit'], c['border'])
    im = imaging.ImagingTemplate(ctx, ap, ip.fixed, wp, gp.fixed, cp).instantiate(
        q, ip, gp, c['vis_block'], 0, c['major'])
    im.ensure_all_bound()
    return im, ip


_shared = {}


def stream(name):
    """The golden coordinates of an end-to-end configuration with integer statistical weights
    (1 to 3), so that the weights accumulated on the grid -- float atomics in any order -- are exact
    and the same in every run; computed once."""
    if name not in _shared:
        c = gi.E2E_CONFIGS[name]
        slices = gi.e2e_inputs(c)['slices']
        rs = np.random.RandomState(5)
        weights = [rs.randint(1, 4, (len(rec), c['P'])).astype(np.float32) for rec in slices]
        _shared[name] = (c, slices, weights)
    return _shared[name]


def feed_weights(im, slices, weights, keep=None):
    im.clear_weights()
    for s, (rec, w) in enumerate(zip(slices, weights)):
        sel = np.ones(len(rec), bool) if keep is None else keep[s]
        uv, w = np.ascontiguousarray(rec.uv[sel]), np.ascontiguousarray(w[sel])
        for i in range(0, len(uv), 500):            # (within every configuration's vis_block)
            im.grid_weights(uv[i:i + 500], w[i:i + 500])
    return im.finalize_weights()


def visited(shape, slices):
    P, H, W = shape
    hit = np.zeros((H, W), bool)
    for rec in slices:
        hit[rec.uv[:, 1] + H // 2, rec.uv[:, 0] + W // 2] = True
    return hit


def moderate_taper(ip):
    """A beam of 6 x 4 pixels at 30 degrees, a cut at 0.7 of the longest baseline of the golden
    tracks (150 m at 0.2 m: 750 wavelengths) with a ramp."""
    return UVTaperParameters((6 * ip.pixel_size, 4 * ip.pixel_size, math.radians(30.0)),
                             min_uv=40.3, max_uv=525.7, inner_tukey=33.0, outer_tukey=100.0)


def test_finalize_weights_natural_with_taper():
    c, slices, weights = stream('degrid')
    plain = moderate_taper(make_params(c)[0])
    im, ip = _imager(c, WeightType.NATURAL, plain)
    assert im.uv_taper == plain and im.grids_weights
    rms, nrms = feed_weights(im, slices, weights)
    got = im.get_buffer('weights_grid')
    T = uv_taper_host(got.shape, ip.image_size, plain)
    hit = visited(got.shape, slices)
    assert np.any(hit & (T > 0)) and np.any(hit & (T == 0))
    d = np.broadcast_to(hit, got.shape).astype(np.float32)
    check_values(got, d, T, d)
    assert rms is not None and np.isfinite(rms) and nrms > 1.0
    # without a taper natural weighting stays the fill with ones
    im0, _ = _imager(c, WeightType.NATURAL, None)
    assert im0.uv_taper is None and not im0.grids_weights
    assert feed_weights(im0, slices, weights) == (None, 1.0)
    np.testing.assert_array_equal(im0.get_buffer('weights_grid'), np.ones(got.shape, np.float32))


@pytest.mark.parametrize('name,weight_type', [('degrid', WeightType.UNIFORM), ('degrid', WeightType.ROBUST),
                                              ('stokes', WeightType.UNIFORM), ('stokes', WeightType.ROBUST)])
def test_finalize_weights_density_with_taper(name, weight_type):
    """Uniform and robust: the tapered grid against the untapered imager's own grid times the twin
    (the robust mean weight is the untapered one: sums of integers, exact in float64)."""
    c, slices, weights = stream(name)
    im0, ip = _imager(c, weight_type, None)
    feed_weights(im0, slices, weights)
    d_dev = im0.get_buffer('weights_grid')
    taper = moderate_taper(ip)
    im, _ = _imager(c, weight_type, taper)
    feed_weights(im, slices, weights)
    got = im.get_buffer('weights_grid')
    T = uv_taper_host(got.shape, ip.image_size, taper)
    assert d_dev.max() <= 1.0
    check_values(got, d_dev, T, d_dev)
    assert np.count_nonzero(got) < np.count_nonzero(d_dev)


def make_psf(im, c, slices, vis_of):
    """The PSF stage of the driver through the host setters; returns (grid of every slice, image)."""
    mid_w = np.arange(c['w_slices']) * float(c['max_w'] / c['wavelength'] / (c['w_slices'] - 0.5))
    grids = []
    im.clear_dirty()
    for s, rec in enumerate(slices):
        im.clear_grid()
        vb = c['vis_block']
        for i in range(0, len(rec), vb):
            chunk = rec[i:i + vb].copy().view(np.recarray)
            im.num_vis = len(chunk)
            im.set_coordinates(chunk)
            im.set_vis(np.ascontiguousarray(vis_of(s)[i:i + vb]).astype(np.complex64))
            im.grid()
        grids.append(im.get_buffer('grid'))
        im.grid_to_image(mid_w[s])
    return grids, im.get_buffer('dirty')


def test_psf_is_that_of_pretapered_weights():
    """Natural weighting with a taper grids the PSF of an untapered natural imager whose statistical
    weights were multiplied by T at each visibility's cell on the host: norm-wise relative error of
    the grids and of the image (before the division by the image-plane taper) at most 1e-5, the
    project's criterion for float32 grids and images."""
    c, slices, weights = stream('degrid')
    im0, ip = _imager(c, WeightType.NATURAL, None)
    taper = moderate_taper(ip)
    im, _ = _imager(c, WeightType.NATURAL, taper)
    feed_weights(im, slices, weights)
    feed_weights(im0, slices, weights)
    P, H, W = im.get_buffer('weights_grid').shape
    T = uv_taper_host((H, W), ip.image_size, taper)
    pre = [w.astype(np.float64) * T[rec.uv[:, 1] + H // 2, rec.uv[:, 0] + W // 2][:, None]
           for rec, w in zip(slices, weights)]
    grids, psf = make_psf(im, c, slices, lambda s: weights[s])
    grids0, psf0 = make_psf(im0, c, slices, lambda s: pre[s])
    for a, b in zip(grids, grids0):
        assert np.abs(b).max() > 0
        assert relerr(a, b) <= 1e-5
    assert tapered_relerr(psf, psf0, kernel_taper(c)) <= 1e-5


def test_normalized_noise():
    """A Gaussian taper raises normalized_noise above 1.  A hard max_uv cut alone gives the figure of
    the same data without the cut visibilities: each of the three sums within n * 2^-53, so
    normalized_noise = sqrt(s2 s0) / s1 within (1/2 + 1/2 + 1) n 2^-53 per run, twice that between
    two runs.  An all-cut taper raises ValueError."""
    c, slices, weights = stream('degrid')
    im, ip = _imager(c, WeightType.NATURAL, UVTaperParameters(8 * c['pixel_size']))
    rms, nrms = feed_weights(im, slices, weights)
    assert nrms > 1.0 and rms > 0
    cut = 400.3
    step = 1.0 / ip.image_size
    keep = [np.hypot(rec.uv[:, 0] * step, rec.uv[:, 1] * step) <= cut for rec in slices]
    assert 0 < sum(int(k.sum()) for k in keep) < sum(len(k) for k in keep)
    n = c['pixels'] ** 2
    for weight_type in (WeightType.NATURAL, WeightType.UNIFORM):
        im_cut, _ = _imager(c, weight_type, UVTaperParameters(max_uv=cut))
        im_all, _ = _imager(c, weight_type, UVTaperParameters())
        got = feed_weights(im_cut, slices, weights)
        want = feed_weights(im_all, slices, weights, keep)
        uncut = feed_weights(im_all, slices, weights)
        for a, b in zip(got, want):
            assert abs(a - b) <= 4 * n * 2.0 ** -53 * b, (weight_type, got, want)
        if weight_type == WeightType.NATURAL:
            assert abs(got[1] - 1.0) <= 4 * n * 2.0 ** -53
        else:
            assert got[1] > 1.0 and abs(got[1] - uncut[1]) > 1e-6
    im_none, _ = _imager(c, WeightType.UNIFORM, UVTaperParameters(min_uv=1.0e6))
    with pytest.raises(ValueError):
        feed_weights(im_none, slices, weights)


def test_process_channels_keeps_the_tapers_apart():
    """Two jobs with different tapers in flight together: each result names its own taper and each
    imager's weights grid is the untapered one times its own twin (to 1e-5: the weights here are
    accumulated by float atomics in whatever order the run takes).  A job that asks for another
    taper than its imager was made with is refused."""
    from katsdpimager_amd import frontend, parameters, preprocess
    ctx, q = context_queue()
    c = gi.E2E_CONFIGS['degrid']
    ip, gp, ap = make_params(c)
    cp = parameters.CleanParameters(c['minor'], c['loop_gain'], c['major_gain'], c['threshold'],
                                    c['mode'], c['psf_cutoff'], c['psf_limit'], c['border'])
    uvw, vis, weights = gi.e2e_raw(c)
    coll = preprocess.VisibilityCollectorDevice(q, [ip, ip], [gp, gp], len(uvw))
    both = np.stack([vis, 0.5 * vis])[:, :, None].astype(np.complex64)
    coll.add(uvw, np.stack([weights, weights]), both, None, None, np.ones((1, 1), np.complex64), None)
    coll.close()
    reader = coll.reader()
    tapers = [UVTaperParameters(5 * ip.pixel_size), UVTaperParameters(max_uv=400.3, outer_tukey=80.0)]
    weight_type = WeightType.ROBUST

    def job(ch, taper):
        im, _ = _imager(c, weight_type, taper, ctx.create_command_queue())
        return dict(reader=reader, rel_channel=ch, imager=im, image_p=ip, grid_p=gp, clean_p=cp,
                    weight_type=weight_type, vis_block=c['vis_block'], major=1, degrid=True)
    plain = job(0, None)
    out = frontend.process_channel(**plain)
    assert out['uv_taper'] is None
    d_dev = plain['imager'].get_buffer('weights_grid').astype(np.float64)
    jobs = [job(ch, taper) for ch, taper in enumerate(tapers)]
    jobs[1]['uv_taper'] = tapers[1]         # (stating it is allowed where it is the imager's)
    results = frontend.process_channels(jobs, workers=2)
    grids = []
    for result, j, taper in zip(results, jobs, tapers):
        assert result['uv_taper'] == taper and result['normalized_noise'] > 1.0
        got = j['imager'].get_buffer('weights_grid')
        want = d_dev * uv_taper_host(got.shape, ip.image_size, taper)
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-30)
        grids.append(got)
    assert relerr(grids[0], grids[1]) > 0.1
    assert results[0]['normalized_noise'] != results[1]['normalized_noise']
    wrong = job(0, tapers[0])
    wrong['uv_taper'] = tapers[1]
    with pytest.raises(ValueError):
        frontend.process_channel(**wrong)
