"""The cases of tests/multiscale_cases.py on the host: that each reaches what it is meant to reach
(every scale, boxes clipped on all sides, a tile index past 1024, the 16-byte and the scalar form of
the residual update under the named buffer layouts), that the lifted workspace layout is the
library's, and that the numpy twin is a trustworthy reference on a non-square image.  No GPU."""
import ctypes

import numpy as np
import pytest

import multiscale_cases as mc

from katsdpimager_amd import multiscale as ms

EPS = 2.0 ** -24


@pytest.mark.parametrize('name', list(mc.CASES))
def test_reference_log_reaches_the_case(name):
    c = mc.CASES[name]
    twin, setup, log = c.reference()
    assert len(log) == c.cycles
    assert sorted(set(log['scale'].tolist())) == list(range(c.K))        # every scale is taken
    assert np.all(log['peak'] > 0)
    # the box of the component's own scale against the image's four sides
    R = 2 * np.array(c.params.radii)[log['scale']]
    bh, bw = c.patch[1] + 2 * R, c.patch[2] + 2 * R
    by0, bx0 = log['y'] - bh // 2, log['x'] - bw // 2
    assert np.any(by0 < 0) and np.any(by0 + bh > c.H)
    assert np.any(bx0 < 0) and np.any(bx0 + bw > c.W)
    if name == 'many_tiles':
        assert c.tiles == (17, 63)
        tile = (log['y'] - c.bp) // 32 * c.tiles[1] + (log['x'] - c.bp) // 32
        assert tile[0] == 1070 and np.sum(tile >= 1024) >= 2 and np.any(tile < 1024)
        # ... and the record of such a tile is the largest of a scale before the first cycle
        for k in range(c.K):
            assert int(np.argmax(setup['tile_max'][k])) >= 1024
    if name == 'tiny':
        assert c.tiles == (1, 1)
        for j in range(1, c.K):
            for k in range(c.K):
                assert c.layout()['cross'][j, k][1] == (c.P, c.H, c.W)      # clipped to the image
    if name == 'six':
        assert c.params.radii[-1] == 64
        lay = c.layout()
        used = set()
        for ks in set(log['scale'].tolist()):
            for j in range(c.K):
                Rjk = c.params.radii[j] + c.params.radii[ks]
                shape = lay['cross'][j, ks][1]
                if shape[1] < c.patch[1] + 2 * Rjk and shape[2] == c.patch[2] + 2 * Rjk:
                    used.add((j, ks))
        assert used, 'no cross patch clipped in y and not in x'
        assert lay['cross'][5, 5][1] == (1, 96, 272)


@pytest.mark.parametrize('name', ['wide', 'tall', 'six'])
def test_aligned_cases_take_the_16_byte_form(name):
    """compact, width = 0 mod 4, border = 0 mod 4: every thread that changes a pixel of any scale
    and plane does so through the 16-byte form, some of them with fewer than four pixels changed
    (the gated store at a box edge).  pitch+1: scale 0 takes both forms within single blocks, the
    scales k >= 1, whose pitch is the width, the 16-byte form still."""
    c = mc.CASES[name]
    log = c.reference()[2]
    assert c.W % 4 == 0 and c.bp % 4 == 0
    forms = mc.forms_taken(c, 'compact', log)
    assert sorted(forms) == [(j, p) for j in range(c.K) for p in range(c.P)]
    for (j, p), n in forms.items():
        assert n['vec'] > 0 and n['partial'] > 0 and n['scalar'] == 0, (j, p, n)
    forms = mc.forms_taken(c, 'pitch+1', log)
    assert mc.pitches(c, 'pitch+1')[1] % 4 == 1
    for (j, p), n in forms.items():
        if j == 0:
            assert n['vec'] > 0 and n['scalar'] > 0 and n['mixed'] > 0 and n['partial'] > 0, (p, n)
        else:
            assert n['vec'] > 0 and n['scalar'] == 0, (j, p, n)
    # aligned rows in a padded plane, and a base that is only 4-byte aligned
    for (j, p), n in mc.forms_taken(c, 'pitch+4', log).items():
        assert n['vec'] > 0 and n['scalar'] == 0, (j, p, n)
    assert mc.pitches(c, 'offset')[0] % 4 != 0
    for (j, p), n in mc.forms_taken(c, 'offset', log).items():
        assert (n['vec'] == 0 and n['scalar'] > 0) if j == 0 else n['scalar'] == 0, (j, p, n)


def test_odd_takes_the_scalar_form_only():
    c = mc.CASES['odd']
    log = c.reference()[2]
    for (j, p), n in mc.forms_taken(c, 'compact', log).items():
        assert n['vec'] == 0 and n['scalar'] > 0, (j, p, n)
    assert (c.H - 2 * c.bp) % 32 and (c.W - 2 * c.bp) % 32              # partial tiles both ways


def test_odd_width_mixes_the_forms_in_the_workspace():
    """At an odd width every fourth row is aligned at compact pitch: both forms within single
    blocks for every scale, the residuals in the workspace included, in every layout."""
    c = mc.CASES['odd_width']
    log = c.reference()[2]
    for layout in mc.LAYOUTS:
        for (j, p), n in mc.forms_taken(c, layout, log).items():
            if j >= 1 or layout == 'compact':
                assert n['vec'] > 0 and n['scalar'] > 0 and n['mixed'] > 0, (layout, j, p, n)


@pytest.mark.parametrize('name', list(mc.CASES))
def test_layout_is_the_library_s(name):
    """ms.workspace_layout against kimg_clean_scales_workspace_bytes, which needs no device."""
    from katsdpimager_amd._lib import lib
    c = mc.CASES[name]
    radii = (ctypes.c_int * c.K)(*c.params.radii)
    nbytes = lib().kimg_clean_scales_workspace_bytes(c.W, c.H, c.P, c.patch[2], c.patch[1], c.bp,
                                                     c.K, radii)
    lay = c.layout()
    assert nbytes == 4 * lay['total'] > 0
    # the sections are in order, 256-byte aligned and do not overlap
    image = (c.P * c.H * c.W + 63) // 64 * 64
    starts = [lay['coef'], lay['taps'], lay['tile_max'], lay['tile_pos']] \
        + [lay['res'][k] for k in range(1, c.K)] \
        + [lay['cross'][j, k][0] for j in range(c.K) for k in range(c.K)]
    assert starts == sorted(starts) and all(s % 64 == 0 for s in starts)
    for k in range(1, c.K):
        assert lay['res'][k] + image <= (lay['res'].get(k + 1) or lay['cross'][0, 0][0])
    last, shape = lay['cross'][c.K - 1, c.K - 1]
    assert last + (int(np.prod(shape)) + 63) // 64 * 64 + 2 * image == lay['total']
    assert lay['tile_pitch'] >= c.tiles[0] * c.tiles[1]


# ---- the twin against float64 on a non-square image ------------------------------------------------

def _conv64(a, taps):
    """conv(a, t) in float64 with the float32 taps as they are, both passes, taps outside the image
    skipped: (value, sum of |t| |t| |a|)."""
    R = (len(taps) - 1) // 2
    t = np.asarray(taps, np.float64)

    def one_pass(v, t):
        n = v.shape[-1]
        out = np.zeros(v.shape)
        for i in range(2 * R + 1):
            lo, hi = max(0, R - i), min(n, n + R - i)
            if lo < hi:
                out[..., lo:hi] += t[i] * v[..., lo - R + i:hi - R + i]
        return out

    def both(v, t):
        return np.swapaxes(one_pass(np.swapaxes(one_pass(v, t), -1, -2), t), -1, -2)
    a = np.asarray(a, np.float64)
    return both(a, t), both(np.abs(a), np.abs(t))


def _conv_bound(R, mag):
    """test_conv_host_against_float64's bound of one pass, (2 R + 2) eps sum |t| |x|, through both:
    the vertical pass adds its own on a temporary that is at most the horizontal magnitude plus
    the horizontal error, and carries the horizontal error through sum |t|."""
    e = (2 * R + 2) * EPS
    return e * (2 + e) * mag


def test_twin_against_float64_on_tall():
    """The twin on `tall` (300 x 72) against the same algorithm in float64 making its own choices:
    the same components in the same order, and every residual within a running bound.  The bound
    starts from the convolution bound above for the set-up (X_jk, n_k, the residuals of the scales
    k >= 1), adds eps |result| for every float32 multiply, divide and subtract, and is carried
    through the cycles: a component's flux inherits the bound of the pixel it is read from, a
    subtraction that of both its operands."""
    c = mc.CASES['tall']
    twin, setup, log = c.reference()
    dirty, psf = c.field()
    H, W, P, K, bp = c.H, c.W, c.P, c.K, c.bp
    ph, pw = c.patch[1], c.patch[2]
    radii = c.params.radii
    gain = float(np.float32(mc.LOOP_GAIN))
    # set-up
    full, efull = {}, {}
    for j in range(K):
        for k in range(j, K):
            v, mag = _conv64(psf, c.params.cross_taps(j, k))
            full[j, k], efull[j, k] = v, _conv_bound(radii[j] + radii[k], mag)
    n = np.array([full[j, j][0, H // 2, W // 2] for j in range(K)])
    en = np.array([efull[j, j][0, H // 2, W // 2] for j in range(K)])
    inv = 1.0 / n
    einv = en / (n * (n - en)) + EPS / (n - en)
    assert np.all(en < 1e-3 * n)

    def scaled(v, ev, j):
        """fl(v32 * inv32[j]) against v inv[j], |v32 - v| <= ev: (value, bound)."""
        t = ev * (inv[j] + einv[j]) + np.abs(v) * einv[j]
        return v * inv[j], t + EPS * (np.abs(v * inv[j]) + t)
    X, EX = {}, {}
    for j in range(K):
        for k in range(K):
            Rjk = radii[j] + radii[k]
            y0, y1 = ms.crop_range(H, ph, Rjk)
            x0, x1 = ms.crop_range(W, pw, Rjk)
            pair = (min(j, k), max(j, k))
            X[j, k], EX[j, k] = scaled(full[pair][:, y0:y1, x0:x1], efull[pair][:, y0:y1, x0:x1], j)
            assert np.all(np.abs(twin.cross[j, k] - X[j, k]) <= EX[j, k])
    res, E = [dirty.astype(np.float64)], [np.zeros(dirty.shape)]
    for k in range(1, K):
        v, mag = _conv64(dirty, c.params.taps[k])
        r, e = scaled(v, _conv_bound(radii[k], mag), k)
        res.append(r)
        E.append(e)
        assert np.all(np.abs(setup['residuals'][k] - r) <= e)
    assert np.all(np.abs(twin.norms - n) <= en + EPS * n)
    # cycles
    biases = c.params.biases.astype(np.float64)
    inner = np.s_[bp:H - bp, bp:W - bp]
    for i in range(c.cycles):
        best = None
        for k in range(K):
            plane = np.abs(res[k][0][inner])
            at = int(np.argmax(plane))
            peak = plane.flat[at]
            if best is None or biases[k] * peak > best[0]:
                best = (biases[k] * peak, k, bp + at // plane.shape[1], bp + at % plane.shape[1], peak)
        _, ks, y, x, peak = best
        assert (ks, y, x) == (log['scale'][i], log['y'][i], log['x'][i]), i
        assert abs(float(log['peak'][i]) - peak) <= E[ks][0, y, x]
        a = gain * res[ks][:, y, x]
        da = gain * E[ks][:, y, x] * (1 + EPS) + EPS * np.abs(a)
        assert np.all(np.abs(log['flux'][i] - a) <= da)
        for j in range(K):
            Rjk = radii[j] + radii[ks]
            bh, bw = ph + 2 * Rjk, pw + 2 * Rjk
            by0, bx0 = y - bh // 2, x - bw // 2
            cy0, cy1 = ms.crop_range(H, ph, Rjk)
            cx0, cx1 = ms.crop_range(W, pw, Rjk)
            y0, y1 = max(0, by0, y - H // 2 + cy0), min(H, by0 + bh, y - H // 2 + cy1)
            x0, x1 = max(0, bx0, x - W // 2 + cx0), min(W, bx0 + bw, x - W // 2 + cx1)
            assert y0 < y1 and x0 < x1
            part = np.s_[:, y0 - y + H // 2 - cy0:y1 - y + H // 2 - cy0,
                         x0 - x + W // 2 - cx0:x1 - x + W // 2 - cx0]
            Xp, EXp = np.abs(X[j, ks][part]), EX[j, ks][part]
            a3, da3 = a[:, None, None], da[:, None, None]
            dp = da3 * Xp + np.abs(a3) * EXp + da3 * EXp
            dp = dp + EPS * (np.abs(a3) * Xp + dp)
            box = np.s_[:, y0:y1, x0:x1]
            res[j][box] -= a3 * X[j, ks][part]
            E[j][box] = (E[j][box] + dp) * (1 + EPS) + EPS * np.abs(res[j][box])
    for j in range(K):
        error = np.abs(twin.residuals[j].astype(np.float64) - res[j])
        print('scale {}: largest error {:.3g}, largest bound {:.3g}, largest residual {:.3g}'.format(
            j, error.max(), E[j].max(), np.abs(res[j]).max()))
        assert np.all(error <= E[j])
