"""Multi-scale CLEAN on the host (katsdpimager_amd/multiscale.py; include/kimg.h, "Multi-scale
CLEAN"): the taps, the numpy twin's convolution against float64, the single scale 0 against the
pinned Hogbom path, and what several scales buy on extended emission.  No GPU."""
import numpy as np
import pytest

import golden_inputs as gi
from oracle import kimg_oracle as orc

from katsdpimager_amd import multiscale as ms
from katsdpimager_amd.parameters import CLEAN_I, CLEAN_SUMSQ

EPS = 2.0 ** -24


# ---- taps ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('scale', [0, 1.5, 4, 9, 30, 50])
def test_taps(scale):
    t = ms.scale_taps(scale)
    R = ms.scale_radius(scale)
    assert t.dtype == np.float32 and len(t) == 2 * R + 1
    if scale:
        assert R == int(np.ceil(3 * scale / (2 * np.sqrt(2 * np.log(2)))))
    else:
        assert R == 0 and t[0] == 1
    np.testing.assert_array_equal(t, t[::-1])
    # every tap is within half an ulp of itself (< eps tap) of a float64 value, and those sum to 1
    assert abs(float(np.sum(t.astype(np.float64))) - 1.0) <= EPS * len(t)
    assert np.argmax(t) == R


def test_cross_taps():
    p = ms.MultiScaleParameters([0, 4, 9])
    assert p.radii == [0, 6, 12]
    for j in range(3):
        for k in range(j, 3):
            t = p.cross_taps(j, k)
            assert t.dtype == np.float32 and len(t) == 2 * (p.radii[j] + p.radii[k]) + 1
            np.testing.assert_array_equal(t, t[::-1])
            assert p.cross_taps(k, j) is t
            assert abs(float(np.sum(t.astype(np.float64))) - 1.0) <= EPS * len(t)
    np.testing.assert_array_equal(p.cross_taps(0, 2), p.taps[2])
    np.testing.assert_array_equal(p.cross_taps(0, 0), [1])
    # default biases: 1 - 0.6 scale / largest, in float64, rounded
    np.testing.assert_array_equal(p.biases, np.array([1.0, 1 - 0.6 * 4 / 9, 1 - 0.6], np.float64)
                                  .astype(np.float32))
    assert ms.MultiScaleParameters([0]).biases.tolist() == [1.0]
    assert ms.MultiScaleParameters([0, 3], biases=[1, 0.25]).biases.tolist() == [1.0, 0.25]


def test_refusals():
    with pytest.raises(ValueError):
        ms.MultiScaleParameters([1, 4])
    with pytest.raises(ValueError):
        ms.MultiScaleParameters([])
    with pytest.raises(ValueError):
        ms.MultiScaleParameters([0, 4, 4])
    with pytest.raises(ValueError):
        ms.MultiScaleParameters([0, 9, 4])
    assert ms.MultiScaleParameters([0, 50]).radii == [0, 64]
    with pytest.raises(ValueError):
        ms.MultiScaleParameters([0, 51])           # radius 65
    assert len(ms.MultiScaleParameters([0, 1, 2, 3, 4, 5])) == 6
    with pytest.raises(ValueError):
        ms.MultiScaleParameters([0, 1, 2, 3, 4, 5, 6])
    with pytest.raises(ValueError):
        ms.MultiScaleParameters([0, 4], biases=[1])
    image = np.zeros((1, 64, 64), np.float32)
    psf = image.copy()
    psf[0, 32, 32] = 1
    p = ms.MultiScaleParameters([0, 4])
    ms.MultiScaleCleanHost(p, 0.0, 0.1, CLEAN_I, image, psf, image.copy())
    with pytest.raises(ValueError):
        ms.MultiScaleCleanHost(p, 0.0, 0.1, CLEAN_SUMSQ, image, psf, image.copy())
    with pytest.raises(ValueError):
        ms.MultiScaleCleanHost(p, 0.0, 0.1, CLEAN_I, image.astype(np.float64),
                               psf.astype(np.float64), image.astype(np.float64))
    with pytest.raises(ValueError):
        ms.conv_host(image.astype(np.float64), [1])
    with pytest.raises(ValueError):
        ms.MultiScaleCleanHost(p, 0.0, 0.1, CLEAN_I, image, psf * np.float32(0.5), image.copy())


def test_c_abi_refusals():
    """KIMG_EUNSUPPORTED before any HIP call: radius, number of scales, mode."""
    import ctypes
    from katsdpimager_amd._lib import lib
    L = lib()
    one = ctypes.c_void_p(16)

    def ints(*v):
        return (ctypes.c_int * len(v))(*v)

    assert L.kimg_image_convolve_separable(one, 8, 64, one, 8, 64, ctypes.c_void_p(32), 8, 64,
                                           8, 8, 1, one, 65, None) == -10002
    assert L.kimg_image_convolve_separable(one, 7, 64, one, 8, 64, ctypes.c_void_p(32), 8, 64,
                                           8, 8, 1, one, 1, None) == -10001
    assert L.kimg_clean_scales_workspace_bytes(64, 64, 1, 9, 9, 1, 2, ints(0, 6)) > 0
    assert L.kimg_clean_scales_workspace_bytes(64, 64, 1, 9, 9, 1, 2, ints(0, 65)) == 0
    assert L.kimg_clean_scales_workspace_bytes(64, 64, 1, 9, 9, 1, 7, ints(0, 1, 2, 3, 4, 5, 6)) == 0
    biases = (ctypes.c_float * 7)(*([1.0] * 7))
    done = ctypes.c_int(0)

    def cycles(mode, K, radii):
        return L.kimg_clean_scales_cycles(one, one, 64, 4096, 64, 64, 1, 9, 9, 1, mode, 0.1, 0.0,
                                          K, radii, biases, 10, None, 0, one, 1 << 30, one,
                                          ctypes.byref(done), None)
    assert cycles(1, 2, ints(0, 6)) == -10002                   # KIMG_CLEAN_SUMSQ
    assert cycles(0, 2, ints(0, 65)) == -10002
    assert cycles(0, 7, ints(0, 1, 2, 3, 4, 5, 6)) == -10002
    assert cycles(0, 2, ints(1, 6)) == -10001                   # scale 0 must be the delta
    assert L.kimg_clean_scales_setup(one, 64, 4096, one, 64, 4096, 64, 64, 1, 9, 9, 1, 2,
                                     ints(0, 65), one, one, 3, None, 0, one, 1 << 30, None) == -10002


# ---- the twin's convolution against float64 ------------------------------------------------------

def _conv64(t):
    """One pass along the last axis in float64: (sum of t[i] in[c - R + i], sum of |t[i]| |in|), taps
    outside the image skipped."""
    R = (len(t) - 1) // 2
    t64 = t.astype(np.float64)

    def one_pass(a):
        a = a.astype(np.float64)
        n = a.shape[-1]
        out = np.zeros(a.shape)
        mag = np.zeros(a.shape)
        for i in range(2 * R + 1):
            lo, hi = max(0, R - i), min(n, n + R - i)
            if lo < hi:
                out[..., lo:hi] += t64[i] * a[..., lo - R + i:hi - R + i]
                mag[..., lo:hi] += abs(t64[i]) * np.abs(a[..., lo - R + i:hi - R + i])
        return out, mag
    return one_pass


@pytest.mark.parametrize('R', [0, 1, 7, 64])
def test_conv_host_against_float64(R):
    """Each pass accumulates 2 R + 1 products in float32: a product and an add are rounded per tap,
    so the running error of a pass is at most (2 R + 2) eps sum |t| |x| (eps = 2^-24) to first
    order.  The vertical pass is checked on the float32 temporary the horizontal pass left (the
    rounding of that temporary is the horizontal pass's own, bounded pass error).  R = 64 exceeds the
    height of 40: taps fall off both edges."""
    rng = np.random.default_rng(100 + R)
    x = rng.standard_normal((2, 40, 70)).astype(np.float32)
    t = rng.standard_normal(2 * R + 1).astype(np.float32)
    one_pass = _conv64(t)
    tmp = ms._conv_axis(x, t)
    ref, mag = one_pass(x)
    assert np.all(np.abs(tmp.astype(np.float64) - ref) <= (2 * R + 2) * EPS * mag)
    got = ms.conv_host(x, t)
    ref, mag = one_pass(np.swapaxes(tmp, -1, -2))
    assert got.dtype == np.float32 and got.shape == x.shape
    assert np.all(np.abs(np.swapaxes(got, -1, -2).astype(np.float64) - ref)
                  <= (2 * R + 2) * EPS * mag)
    if R == 0:
        np.testing.assert_array_equal(ms.conv_host(x, [1]), x)


# ---- the single scale 0 is the Hogbom path ---------------------------------------------------------

@pytest.mark.parametrize('name', [n for n, c in gi.CLEAN_CONFIGS.items() if c['mode'] == CLEAN_I])
def test_single_scale_is_hogbom(golden, name):
    c = gi.CLEAN_CONFIGS[name]
    g = golden('g7_clean_' + name)
    ci = gi.clean_inputs(c)
    dirty, model = ci['dirty'].copy(), np.zeros_like(ci['dirty'])
    ref = orc.Clean(c['pixels'], c['border'], c['loop_gain'], c['mode'], dirty, ci['psf'], model)
    ref.reset()
    values, pos, pix = [], [], []
    for i in range(c['cycles']):
        v, p, m = ref(ci['psf_patch'], c['threshold'])
        if v is None:
            break
        values.append(v)
        pos.append(ref.last_pos)
        pix.append(m)
    assert len(values) == len(g['values']) > 10
    dirty2, model2 = ci['dirty'].copy(), np.zeros_like(ci['dirty'])
    twin = ms.MultiScaleCleanHost(ms.MultiScaleParameters([0]), c['border'], c['loop_gain'],
                                  c['mode'], dirty2, ci['psf'], model2)
    twin.reset()
    twin.prepare(ci['psf_patch'])
    np.testing.assert_array_equal(twin.tile_max[0], g['tile_max0'])
    np.testing.assert_array_equal(twin.tile_pos[0], g['tile_pos0'])
    log = twin.run_cycles(ci['psf_patch'], c['threshold'], c['cycles'])
    assert len(log) == len(values)
    assert np.all(log['scale'] == 0)
    np.testing.assert_array_equal(np.stack([log['y'], log['x']], axis=1), np.array(pos, np.int32))
    np.testing.assert_array_equal(log['peak'], np.array(values, np.float32))
    np.testing.assert_array_equal(log['flux'], np.array(pix, np.float32))
    np.testing.assert_array_equal(dirty2, dirty)
    np.testing.assert_array_equal(model2, model)
    np.testing.assert_array_equal(twin.tile_max[0], ref._tile_max)
    np.testing.assert_array_equal(twin.tile_pos[0], ref._tile_pos)


# ---- physics ----------------------------------------------------------------------------------------

def extended_field(G=128):
    """Three Gaussian blobs (FWHM 9, 4 and a point) convolved with a Gaussian-core PSF: (dirty,
    psf, true flux), float32 [1][G][G], noise-free."""
    yy, xx = np.mgrid[:G, :G].astype(np.float64)

    def blob(y, x, fwhm, flux):
        if fwhm == 0:
            out = np.zeros((G, G))
            out[y, x] = flux
            return out
        s = fwhm / (2 * np.sqrt(2 * np.log(2)))
        g = np.exp(-((yy - y) ** 2 + (xx - x) ** 2) / (2 * s * s))
        return flux * g / g.sum()
    sky = blob(40, 44, 9, 30.0) + blob(84, 50, 4, 12.0) + blob(60, 92, 0, 3.0)
    c = G // 2
    core = np.exp(-((yy - c) ** 2 + (xx - c) ** 2) / (2 * 1.5 ** 2))
    wings = 0.02 * np.cos(0.7 * np.hypot(yy - c, xx - c)) * np.exp(-np.hypot(yy - c, xx - c) / 25.0)
    psf = core + wings * (1 - core)
    psf /= psf[c, c]
    f = np.fft.fft2
    dirty = np.real(np.fft.ifft2(f(sky) * f(np.fft.ifftshift(psf))))
    psf32 = psf.astype(np.float32)[np.newaxis]
    assert psf32[0, c, c] == 1
    return dirty.astype(np.float32)[np.newaxis], psf32, float(sky.sum())


def _run_host(scales, cycles=60, gain=0.1):
    dirty, psf, flux = extended_field()
    model = np.zeros_like(dirty)
    border = 0.05
    twin = ms.MultiScaleCleanHost(ms.MultiScaleParameters(scales), border, gain, CLEAN_I, dirty,
                                  psf, model)
    twin.reset()
    log = twin.run_cycles((1, 41, 41), 0.0, cycles)
    bp = twin.border_pixels
    inner = dirty[0, bp:-bp, bp:-bp].astype(np.float64)
    return float(np.sqrt(np.mean(inner ** 2))), float(model.astype(np.float64).sum()), flux, log


def test_scales_beat_deltas_on_extended_emission():
    """60 cycles at gain 0.1: with the scales [0, 4, 9] the residual inside the border is smaller
    than with deltas alone (the measured ratio, 0.185, is in DESIGN.md 5.13; none is asserted).  The
    model flux of this three-source field is printed only (41.8 of 45 after 60 shared cycles): the
    1 - 0.9^60 fraction holds for an isolated source, where the next test asserts it."""
    rms_ms, flux_ms, true_flux, log = _run_host([0, 4, 9])
    rms_delta, flux_delta, _, _ = _run_host([0])
    print('residual rms: scales [0, 4, 9] {:.6g}, [0] {:.6g}, ratio {:.4f}; model flux {:.5g} and '
          '{:.5g} of {:.5g}; scales taken {}'.format(
              rms_ms, rms_delta, rms_ms / rms_delta, flux_ms, flux_delta, true_flux,
              np.bincount(log['scale'], minlength=3).tolist()))
    assert len(log) == 60
    assert rms_ms < rms_delta


def test_model_flux_of_an_isolated_source():
    """An isolated source of the scale's own shape loses the fraction `gain` of what is left per
    cycle: after 60 cycles the model holds 1 - 0.9^60 of its flux, to 1 %."""
    G, c = 128, 64
    yy, xx = np.mgrid[:G, :G].astype(np.float64)
    s = 9 / (2 * np.sqrt(2 * np.log(2)))
    sky = np.exp(-((yy - 60) ** 2 + (xx - 70) ** 2) / (2 * s * s))
    sky *= 25.0 / sky.sum()
    psf = np.exp(-((yy - c) ** 2 + (xx - c) ** 2) / (2 * 1.5 ** 2))
    dirty = np.real(np.fft.ifft2(np.fft.fft2(sky) * np.fft.fft2(np.fft.ifftshift(psf))))
    dirty = dirty.astype(np.float32)[np.newaxis]
    psf = psf.astype(np.float32)[np.newaxis]
    model = np.zeros_like(dirty)
    twin = ms.MultiScaleCleanHost(ms.MultiScaleParameters([0, 4, 9]), 0.05, 0.1, CLEAN_I, dirty,
                                  psf, model)
    twin.reset()
    log = twin.run_cycles((1, 25, 25), 0.0, 60)
    assert len(log) == 60
    expected = (1 - 0.9 ** 60) * 25.0
    got = float(model.astype(np.float64).sum())
    print('model flux {:.6g}, expected {:.6g}'.format(got, expected))
    assert abs(got - expected) <= 0.01 * expected
