"""The float64 path (the reference's --precision double): gridder, degridder, grid <-> image and the
image-plane operators on complex128 / float64 arrays (include/kimg.h, "float64 path").

Truths are numpy restatements of the arithmetic contract of include/kimg.h:
  gridder    s = float32(vis * wgt), then in double grid[v0 + j][u0 + k] += (s conj(kv_j)) conj(ku_k);
  degridder  complex64(vis - weight * sum_k ku_k sum_j kv_j g[j][k]), evaluated in double.
The bar on real-valued data is 1e-12 of the truth's peak, which a float32 accumulator misses by
orders of magnitude; on integer data with partial sums above 2^24 (and below 2^53) the kernels must
equal the truth bit for bit.  CPU tests (no marker) check the operator surface and the ISA."""
import ctypes
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import golden_inputs as gi                                              # noqa: E402
from helpers import context_queue, grid_to_image_truth, tapered_relerr  # noqa: E402
from test_exact_gridding import Case, Padded, _dev, _inputs, _stream, grid_truth, degrid_truth  # noqa: E402

KIMG_EUNSUPPORTED = -10002
EXACT32 = float(1 << 24)
EXACT64 = float(1 << 53)
VARIANT = {'auto': 0, 'generic': 1, 'mfma': 2, 'binned': 3}


# ---------------------------------------------------------------------------------------------
# numpy truths of the contract

def _valid(uv, w_plane, G, OV, W):
    half = G // 2
    u, v, su, sv = (uv[:, i].astype(np.int64) for i in range(4))
    wp = w_plane.astype(np.int64)
    return ((u + half >= 0) & (u + half < G) & (v + half >= 0) & (v + half < G) & (su >= 0)
            & (su < OV) & (sv >= 0) & (sv < OV) & (wp >= 0) & (wp < W))


def grid_truth64(kern, uv, w_plane, vis, wg):
    """The gridder's contract in numpy: [P][G][G] complex128."""
    W, OV, K = kern.shape
    P, G = wg.shape[0], wg.shape[-1]
    ok = _valid(uv, w_plane, G, OV, W)
    uv, w_plane, vis = uv[ok].astype(np.int64), w_plane[ok].astype(np.int64), vis[ok]
    half = G // 2
    bias = (K - 1) // 2 - half
    u, v = uv[:, 0], uv[:, 1]
    kern = kern.astype(np.complex128)
    kv = np.conj(kern[w_plane, uv[:, 3]])
    ku = np.conj(kern[w_plane, uv[:, 2]])
    x = (u - bias)[:, None] + np.arange(K)[None, :]
    xin = (x >= 0) & (x < G)
    out = np.zeros((P, G * G), np.complex128)
    for p in range(P):
        w = wg[p][v + half, u + half]
        s = (vis[:, p].real * w).astype(np.float32) + 1j * (vis[:, p].imag * w).astype(np.float32)
        for j in range(K):
            y = v - bias + j
            a = s.astype(np.complex128) * kv[:, j]
            val = a[:, None] * ku
            m = xin & ((y >= 0) & (y < G))[:, None]
            idx = (y[:, None] * G + x)[m]
            out[p] += np.bincount(idx, val.real[m], G * G) + 1j * np.bincount(idx, val.imag[m], G * G)
    return out.reshape(P, G, G)


def degrid_truth64(kern, uv, w_plane, weights, vis0, grid):
    """The degridder's contract before its final rounding: complex128 [N][P]."""
    W, OV, K = kern.shape
    P, G = grid.shape[0], grid.shape[-1]
    ok = _valid(uv, w_plane, G, OV, W)
    out = vis0.astype(np.complex128).copy()
    uv, wp = uv[ok].astype(np.int64), w_plane[ok].astype(np.int64)
    bias = (K - 1) // 2 - G // 2
    kern = kern.astype(np.complex128)
    kv, ku = kern[wp, uv[:, 3]], kern[wp, uv[:, 2]]
    x = (uv[:, 0] - bias)[:, None] + np.arange(K)[None, :]
    g = np.zeros((P, G + 2 * K, G + 2 * K), np.complex128)     # zero margin: taps off the grid
    g[:, K:K + G, K:K + G] = grid
    pred = np.zeros((len(uv), P), np.complex128)
    for j in range(K):
        y = uv[:, 1] - bias + j
        for p in range(P):
            pred[:, p] += kv[:, j] * np.sum(ku * g[p][(y + K)[:, None], x + K], axis=1)
    out[ok] -= weights[ok].astype(np.float64) * pred
    return out


# ---------------------------------------------------------------------------------------------
# inputs and C ABI runs

def _real_table(rs, W, OV, K):
    return (rs.standard_normal((W, OV, K)) + 1j * rs.standard_normal((W, OV, K))).astype(np.complex64)


def _real_inputs(K, P, W, stream, n, G, seed, OV=8, bad=True):
    """Random real-valued data on a stream of test_exact_gridding's kinds, plus (bad=True) records
    whose cell, sub-cell or plane is out of range, and footprints hanging over the edges."""
    rs = np.random.RandomState(seed)
    bias = (K - 1) // 2 - G // 2
    xy = _stream(stream, rs, n, G, K).astype(np.int64)
    sub = rs.randint(0, OV, (len(xy), 2))
    wp = rs.randint(0, W, len(xy))
    uv = np.concatenate([xy + bias, sub], axis=1)
    if bad:
        extra = []
        half = G // 2
        for u, v, su, sv, w in ((half, 0, 0, 0, 0), (0, -half - 1, 1, 1, 0), (0, 0, OV, 0, 0),
                                (0, 0, 0, -1, 0), (0, 0, 0, 0, W), (3, 4, 1, 2, -1),
                                (-half, -half, 2, 3, 0), (half - 1, half - 1, 3, 2, W - 1),
                                (-half + 2, half - 3, 1, 1, 0)):
            extra.append((u, v, su, sv, w))
        extra = np.array(extra, np.int64)
        uv = np.concatenate([uv, extra[:, :4]])
        wp = np.concatenate([wp, extra[:, 4]])
    N = len(uv)
    vis = (rs.standard_normal((N, P)) + 1j * rs.standard_normal((N, P))).astype(np.complex64)
    wg = rs.uniform(0.5, 2.0, (P, G, G)).astype(np.float32)
    return dict(kern=_real_table(rs, W, OV, K), uv=uv.astype(np.int16), w_plane=wp.astype(np.int16),
                vis=vis, wg=wg, weights=rs.uniform(0.5, 1.5, (N, P)).astype(np.float32),
                grid=(rs.standard_normal((P, G, G)) + 1j * rs.standard_normal((P, G, G))))


def _lib():
    from katsdpimager_amd._lib import lib
    return lib()


_keep = []


def _binned_ws(ctx, variant, nbytes):
    """Scratch of the binned variant (the float32 sizes, include/kimg.h); None elsewhere."""
    from katsdpimager_amd import accel
    if variant != 'binned' or not nbytes:
        return None, 0
    ws = accel.DeviceArray(ctx, (int(nbytes),), np.uint8)
    _keep[:] = [ws]
    return ws.ptr, int(nbytes)


def variants(K):
    """Every variant that runs a different kernel at width K: the window kernel (mfma), the same
    over sorted copies (binned), and the generic kernel; widths above 32 have only the last."""
    return ('generic', 'mfma', 'binned') if K <= 32 else ('generic', 'auto')


def run_grid64(inp, variant='generic', prefill=None, rpad=0, vpad=0, wg_pad=(0, 0)):
    from katsdpimager_amd._lib import check
    ctx, q = context_queue()
    W, OV, K = inp['kern'].shape
    P, G = inp['wg'].shape[0], inp['wg'].shape[-1]
    n = len(inp['uv'])
    g0 = np.zeros((P, G, G), np.complex128) if prefill is None else prefill.astype(np.complex128)
    g = Padded(ctx, q, g0, rpad, vpad, np.complex128(-1.5e7 + 3.25e6j))
    wg = Padded(ctx, q, inp['wg'], wg_pad[0], wg_pad[1], np.float32(1e6))
    table = _dev(ctx, q, inp['kern'])
    uv, wp, vis = _dev(ctx, q, inp['uv']), _dev(ctx, q, inp['w_plane']), _dev(ctx, q, inp['vis'])
    ws, nbytes = _binned_ws(ctx, variant, _lib().kimg_grid_binned_workspace_bytes(n, P, W, OV, K))
    rc = _lib().kimg_grid_f64(g.dev.ptr, g.row, g.pol, G, P, wg.dev.ptr, wg.row, wg.pol, uv.ptr,
                              wp.ptr, vis.ptr, n, table.ptr, W, OV, K, ws, nbytes, VARIANT[variant],
                              q.handle)
    check(rc, 'kimg_grid_f64 ' + variant)
    q.finish()
    wg.get(q)
    return g.get(q)


def run_degrid64(inp, variant='generic', rpad=0, vpad=0):
    from katsdpimager_amd._lib import check
    ctx, q = context_queue()
    W, OV, K = inp['kern'].shape
    P, G = inp['grid'].shape[0], inp['grid'].shape[-1]
    n = len(inp['uv'])
    g = Padded(ctx, q, inp['grid'].astype(np.complex128), rpad, vpad, np.complex128(3e6 - 5e6j))
    table = _dev(ctx, q, inp['kern'])
    uv, wp = _dev(ctx, q, inp['uv']), _dev(ctx, q, inp['w_plane'])
    weights, vis = _dev(ctx, q, inp['weights']), _dev(ctx, q, inp['vis'])
    ws, nbytes = _binned_ws(ctx, variant, _lib().kimg_degrid_binned_workspace_bytes(n, P, W, OV, K))
    rc = _lib().kimg_degrid_f64(g.dev.ptr, g.row, g.pol, G, P, uv.ptr, wp.ptr, weights.ptr,
                                vis.ptr, n, table.ptr, W, OV, K, ws, nbytes, VARIANT[variant],
                                q.handle)
    check(rc, 'kimg_degrid_f64 ' + variant)
    q.finish()
    g.get(q)
    return vis.get(q)


def _peak_err(got, want):
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


# ---------------------------------------------------------------------------------------------
# CPU: operator surface, ABI, ISA

def _fixed64(P=1):
    from katsdpimager_amd import parameters
    return parameters.FixedImageParameters(list(range(P)), np.float64)


def _fixed_grid():
    from katsdpimager_amd import parameters
    return parameters.FixedGridParameters(7.0, 8, 4, 5.0, 28)


def test_templates_accept_float64():
    from katsdpimager_amd import grid, image
    for T in (grid.GridderTemplate, grid.DegridderTemplate):
        t = T(None, _fixed64(), _fixed_grid())
        assert t.variant == grid.GRID_VARIANTS['auto']
        assert T(None, _fixed64(), _fixed_grid(), {'variant': 'generic'}).variant == 1
    gi_t = image.GridImageTemplate(None, np.float64, {'real_transform': True, 'own_transform': True})
    assert gi_t.layer_to_image.real_dtype == np.float64
    for T in (image.ScaleTemplate, image.AddImageTemplate, image.ApplyPrimaryBeamTemplate):
        assert T(None, np.float64, 2).dtype == np.float64
    for T in (image.LayerToImageTemplate, image.ImageToLayerTemplate):
        assert T(None, np.float64).real_dtype == np.float64


def test_float64_tuning_limits():
    from katsdpimager_amd import grid
    for T in (grid.GridderTemplate, grid.DegridderTemplate):
        for tuning in ({'arith': 'split_fp16'}, {'arith': 'fp32_32x32'},
                       {'arith': 'split_fp16', 'variant': 'mfma'}):
            if T is grid.DegridderTemplate and tuning.get('arith') == 'fp32_32x32':
                continue
            with pytest.raises(ValueError):
                T(None, _fixed64(), _fixed_grid(), tuning)
        for v in ('auto', 'generic', 'mfma', 'binned'):
            assert T(None, _fixed64(), _fixed_grid(), {'arith': 'fp32', 'variant': v}).variant == \
                grid.GRID_VARIANTS[v]
    # float32 keeps every form
    from katsdpimager_amd import parameters
    f32 = parameters.FixedImageParameters([0], np.float32)
    assert grid.GridderTemplate(None, f32, _fixed_grid(), {'arith': 'split_fp16',
                                                          'variant': 'binned'}).arith == 1


def test_out_of_scope_templates_reject_float64():
    from katsdpimager_amd import clean, imaging, parameters, predict, types, weight
    with pytest.raises(ValueError):
        types.require_float32(np.float64, 'x')
    types.require_float32_or_64(np.float64, 'x')
    with pytest.raises(ValueError):
        types.require_float32_or_64(np.float16, 'x')
    cp = parameters.CleanParameters(100, 0.1, 0.85, 5.0, 0, 0.01, 0.5, 8)
    with pytest.raises(ValueError):
        clean.CleanTemplate(None, cp, np.float64, 1)
    with pytest.raises(ValueError):
        clean.PsfPatchTemplate(None, np.float64, 1)
    with pytest.raises(ValueError):
        clean.NoiseEstTemplate(None, np.float64, 1)
    with pytest.raises(ValueError, match='PredictTemplate'):
        predict.PredictTemplate(None, np.float64, 1)
    wp = parameters.WeightParameters(weight.WeightType.NATURAL, 0.0)
    ap = parameters.ArrayParameters(13.5, 100.0)
    with pytest.raises(ValueError, match='ImagingTemplate'):
        imaging.ImagingTemplate(None, ap, _fixed64(), wp, _fixed_grid(), cp)


def test_f64_abi_declared_exported_and_bound():
    import re
    from katsdpimager_amd import _lib, build
    build.build_lib()
    header = open(os.path.join(ROOT, 'include', 'kimg.h')).read()
    names = {'kimg_grid_f64', 'kimg_degrid_f64', 'kimg_grid_to_layer_f64', 'kimg_layer_to_grid_f64',
             'kimg_layer_to_image_f64', 'kimg_image_to_layer_f64', 'kimg_fft_plan_create_f64',
             'kimg_scale_f64', 'kimg_add_image_f64', 'kimg_apply_primary_beam_f64'}
    declared = set(re.findall(r'\b(kimg_[a-z0-9_]+)\s*\(', header))
    assert names <= declared and names <= set(_lib.PROTOTYPES)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(handle, n), n
    assert _lib.lib().kimg_version() == _lib.VERSION == 5
    L = _lib.lib()
    one = ctypes.c_void_p(1)
    # argument checks before any HIP call: the window variants take widths up to 32, a bad variant
    # is invalid
    for variant, rc in ((2, KIMG_EUNSUPPORTED), (3, KIMG_EUNSUPPORTED), (7, -10001)):
        assert L.kimg_grid_f64(one, 64, 4096, 64, 1, one, 64, 4096, one, one, one, 4, one, 1, 8, 40,
                               None, 0, variant, None) == rc
        assert L.kimg_degrid_f64(one, 64, 4096, 64, 1, one, one, one, one, 4, one, 1, 8, 40, None,
                                 0, variant, None) == rc
    assert L.kimg_grid_f64(one, 8, 64, 8, 5, one, 8, 64, one, one, one, 4, one, 1, 8, 4, None, 0,
                           0, None) == KIMG_EUNSUPPORTED


def test_f64_gridder_isa_uses_f64_atomics_without_cas():
    """The gridder's atomics lower to global_atomic_add_f64 with no compare-and-swap loop (the
    library's flags, -munsafe-fp-atomics)."""
    from katsdpimager_amd import build
    src = os.path.join(ROOT, 'katsdpimager_amd', 'csrc', 'grid_f64.hip')
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.check_call([build.hipcc()] + build.FLAGS + ['--save-temps', '-c', src, '-o',
                                                               os.path.join(tmp, 'g.o')], cwd=tmp)
        asm = open(glob.glob(os.path.join(tmp, '*gfx950*.s'))[0]).read()
    assert asm.count('global_atomic_add_f64') > 0
    assert 'cmpswap' not in asm.lower()


def test_truths_restate_the_contract():
    """The numpy truths agree with test_exact_gridding's independent truths on integer data."""
    c = Case('f64_self', 8, 4, 4, 2, 'slow', 500)
    inp = _inputs(c)
    want, _ = grid_truth(inp['kern'], inp['uv'], inp['w_plane'], inp['vis'], inp['wg'])
    assert np.array_equal(grid_truth64(inp['kern'], inp['uv'], inp['w_plane'], inp['vis'],
                                       inp['wg']), want[:, 1:-1, 1:-1])
    d = _inputs(c, degrid=True)
    want, _ = degrid_truth(d['kern'], d['uv'], d['w_plane'], d['weights'], d['vis'], d['grid'])
    assert np.array_equal(degrid_truth64(d['kern'], d['uv'], d['w_plane'], d['weights'], d['vis'],
                                         d['grid']), want)


# ---------------------------------------------------------------------------------------------
# GPU: reference goldens

@pytest.mark.gpu
@pytest.mark.parametrize('variant', ['generic', 'mfma', 'binned', 'auto'])
def test_golden_grid_p1_f64(golden, variant):
    from oracle import kimg_oracle as orc
    c = gi.GRID_CONFIGS['p1_f64']
    t = gi.grid_track(c)
    kernel, _ = orc.convolution_kernel(c['cell_size'], c['wavelength'], c['max_w'], c['w_slices'],
                                       c['w_planes'], c['oversample'], c['kernel_width'],
                                       c['antialias_width'], c['image_oversample'])
    G = c['pixels']
    wg = np.zeros((c['P'], G, G), np.float32)
    gi.middle(wg, t['weights_grid'].shape)[:] = t['weights_grid']
    inp = dict(kern=kernel, uv=np.concatenate((t['uv'], t['sub_uv']), axis=1), w_plane=t['w_plane'],
               vis=t['vis'], wg=wg)
    got = run_grid64(inp, variant)
    expected = golden('g2_grid_p1_f64')['grid']
    assert expected.dtype == np.complex128
    assert _peak_err(got, expected) < 1e-7


@pytest.mark.gpu
@pytest.mark.parametrize('variant', ['generic', 'mfma', 'binned', 'auto'])
def test_golden_degrid_p1_f64(golden, variant):
    from oracle import kimg_oracle as orc
    c = gi.GRID_CONFIGS['p1_f64']
    t = gi.grid_track(c)
    dg = gi.degrid_inputs(c)
    kernel, _ = orc.convolution_kernel(c['cell_size'], c['wavelength'], c['max_w'], c['w_slices'],
                                       c['w_planes'], c['oversample'], c['kernel_width'],
                                       c['antialias_width'], c['image_oversample'])
    inp = dict(kern=kernel, uv=np.concatenate((t['uv'], t['sub_uv']), axis=1), w_plane=t['w_plane'],
               weights=dg['weights'], vis=dg['vis'], grid=dg['grid'])
    assert dg['grid'].dtype == np.complex128
    got = run_degrid64(inp, variant)
    expected = golden('g3_degrid_p1_f64')['residual']
    np.testing.assert_allclose(got, expected, rtol=1e-6, atol=1e-6 * np.abs(expected).max())


# ---------------------------------------------------------------------------------------------
# GPU: float64 truth on random data

TRUTH_CASES = [
    # (K, P, W, stream, n, G)
    (8, 1, 32, 'slow', 3001, 160),
    (8, 4, 300, 'jumps', 0, 160),
    (28, 2, 32, 'edges', 0, 168),
    (28, 1, 300, 'random', 2001, 168),
    (28, 4, 32, 'slow', 1023, 168),
    (60, 1, 32, 'sweep', 0, 200),
    (60, 2, 300, 'slow', 777, 200),
    (60, 4, 32, 'jumps', 0, 200),
    (8, 2, 32, 'slow', 1, 160),
    (28, 1, 32, 'slow', 65, 168),
    (28, 3, 32, 'random', 1501, 168),
]


def _truth_id(c):
    return 'k%d_p%d_w%d_%s_%d' % c[:5]


@pytest.mark.gpu
@pytest.mark.parametrize('case', TRUTH_CASES, ids=_truth_id)
def test_grid_f64_vs_truth(case):
    K, P, W, stream, n, G = case
    inp = _real_inputs(K, P, W, stream, n, G, seed=K * 100 + P * 10 + (W > 32))
    want = grid_truth64(inp['kern'], inp['uv'], inp['w_plane'], inp['vis'], inp['wg'])
    for variant in variants(K):
        got = run_grid64(inp, variant)
        assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)), variant
    # a prefilled grid with padded strides: the gridder adds, the padding is left alone
    rs = np.random.RandomState(9)
    pre = rs.standard_normal(want.shape) + 1j * rs.standard_normal(want.shape)
    for variant in variants(K):
        got = run_grid64(inp, variant, prefill=pre, rpad=5, vpad=3, wg_pad=(3, 1))
        assert np.max(np.abs(got - (want + pre))) <= 1e-12 * np.max(np.abs(want + pre)), variant


@pytest.mark.gpu
@pytest.mark.parametrize('case', TRUTH_CASES, ids=_truth_id)
def test_degrid_f64_vs_truth(case):
    K, P, W, stream, n, G = case
    inp = _real_inputs(K, P, W, stream, n, G, seed=K * 100 + P * 10 + (W > 32) + 7)
    want = degrid_truth64(inp['kern'], inp['uv'], inp['w_plane'], inp['weights'], inp['vis'],
                          inp['grid'])
    for variant in variants(K):
        got = run_degrid64(inp, variant, 3, 2)
        # one final rounding to complex64 of the double result
        np.testing.assert_array_equal(got, want.astype(np.complex64), err_msg=variant)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', ['mfma', 'binned'])
def test_window_variants_refuse_widths_above_32(variant):
    """Widths 33 and up run the generic kernels only (include/kimg.h)."""
    from katsdpimager_amd._lib import KimgError
    inp = _real_inputs(40, 1, 4, 'slow', 10, 128, 1)
    with pytest.raises(KimgError) as e:
        run_grid64(inp, variant)
    assert e.value.code == KIMG_EUNSUPPORTED
    with pytest.raises(KimgError) as e:
        run_degrid64(inp, variant)
    assert e.value.code == KIMG_EUNSUPPORTED


# ---------------------------------------------------------------------------------------------
# GPU: exact integer data beyond float32's 2^24

EXACT_CASES = [Case('x8_p2', 8, 4, 4, 2, 'slow', 3000), Case('x28_hbm', 28, 8, 48, 1, 'slow', 2000),
               Case('x60_p4', 60, 8, 4, 4, 'jumps'), Case('x28_edges_p3', 28, 4, 4, 3, 'edges'),
               Case('x32_p4_moves', 32, 8, 4, 4, 'moves'), Case('x16_sweep', 16, 8, 4, 1, 'sweep')]


@pytest.mark.gpu
@pytest.mark.parametrize('case', EXACT_CASES, ids=repr)
def test_grid_f64_exact_beyond_2_24(case):
    inp = _inputs(case)
    # an odd scale: the samples stay exact in float32 (|vis * wgt| <= 3 * 40009 * 3 < 2^24), the
    # sums leave float32's reach (a power of two would only move the exponent)
    inp['vis'] = (inp['vis'] * np.float32(40009)).astype(np.complex64)
    want, bound = grid_truth(inp['kern'], inp['uv'], inp['w_plane'], inp['vis'], inp['wg'])
    want, bound = want[:, 1:-1, 1:-1], bound[:, 1:-1, 1:-1]
    assert bound.max() > EXACT32 and bound.max() < EXACT64
    assert not np.array_equal(want.astype(np.complex64).astype(np.complex128), want)
    for variant in variants(case.K):
        assert np.array_equal(run_grid64(inp, variant), want), variant


@pytest.mark.gpu
@pytest.mark.parametrize('case', EXACT_CASES, ids=repr)
def test_degrid_f64_exact_beyond_2_24(case):
    inp = _inputs(case, degrid=True)
    inp['grid'] = inp['grid'].astype(np.complex128) * 1000003.0     # (odd, as above)
    want, bound = degrid_truth(inp['kern'], inp['uv'], inp['w_plane'], inp['weights'], inp['vis'],
                               inp['grid'])
    assert bound.max() > EXACT32 and bound.max() < EXACT64
    for variant in variants(case.K):
        np.testing.assert_array_equal(run_degrid64(inp, variant), want.astype(np.complex64),
                                      err_msg=variant)


@pytest.mark.gpu
@pytest.mark.parametrize('case', EXACT_CASES[:3], ids=repr)
def test_adjoint(case):
    """<degrid(G), v> = <G, grid(v)> in double.  The degridder returns complex64, so the table,
    grid and visibilities are integers whose predictions stay exactly representable; the grid
    (not the predictions) is large enough that float32 accumulation in the gridder would not be."""
    inp = _inputs(case, degrid=True)
    P, G = case.P, case.G
    v = inp['vis']
    # gridder: unit density weights, so grid(v) is the adjoint of the unit-weight degridder
    ginp = dict(inp, wg=np.ones((P, G, G), np.float32), vis=v)
    dinp = dict(inp, weights=np.ones_like(inp['weights']), vis=np.zeros_like(v))
    for variant in variants(case.K):
        gv = run_grid64(ginp, variant)
        pred = -run_degrid64(dinp, variant).astype(np.complex128)
        lhs = np.vdot(pred, v.astype(np.complex128))
        rhs = np.vdot(inp['grid'].astype(np.complex128), gv)
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs)), variant
        assert abs(lhs) > 0


# ---------------------------------------------------------------------------------------------
# GPU: grid <-> image and the image-plane operators

def _grid_image_ops(G, Gg, P, lm_scale, lm_bias):
    from katsdpimager_amd import image
    ctx, q = context_queue()
    t = image.GridImageTemplate(ctx, np.float64)
    plan = t.make_fft_plan((G, G))
    g2i = t.instantiate_grid_to_image(q, (P, Gg, Gg), lm_scale, lm_bias, plan)
    g2i.ensure_all_bound()
    i2g = t.instantiate_image_to_grid(q, (P, Gg, Gg), lm_scale, lm_bias, plan)
    i2g.bind(layer=g2i.buffer('layer'), image=g2i.buffer('image'), kernel1d=g2i.buffer('kernel1d'))
    i2g.ensure_all_bound()
    return q, g2i, i2g


def image_to_grid_truth(image, kernel1d, lm_scale, lm_bias, w, Gg):
    """ImageToGrid in numpy float64: image / (taper n) e^{-2 pi i w (n-1)}, shifted, forward FFT,
    corners -> centred grid."""
    P, G, _ = image.shape
    x = np.arange(G) * lm_scale + lm_bias
    l, m = x[None, :], x[:, None]
    n = np.sqrt(1.0 - (m * m + l * l))
    r = w * (n - 1.0)
    r = r - np.rint(r)
    phase = np.exp(-2j * np.pi * r)
    taper = np.outer(kernel1d, kernel1d)
    out = np.zeros((P, Gg, Gg), np.complex128)
    for p in range(P):
        layer = np.fft.fft2(np.fft.ifftshift(image[p] / (taper * n) * phase))
        out[p] = np.fft.fftshift(layer)[G // 2 - Gg // 2:G // 2 + Gg // 2,
                                        G // 2 - Gg // 2:G // 2 + Gg // 2]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('w', [0.0, 37.5])
def test_grid_image_f64_vs_numpy(w):
    from oracle import kimg_oracle as orc
    G, Gg, P = 256, 192, 2
    lm_scale = 1.5e-3
    lm_bias = -0.5 * G * lm_scale
    q, g2i, i2g = _grid_image_ops(G, Gg, P, lm_scale, lm_bias)
    rs = np.random.RandomState(4)
    grid = rs.standard_normal((P, Gg, Gg)) + 1j * rs.standard_normal((P, Gg, Gg))
    k1d = orc.taper(G, 7.0, orc.kernel_beta(7.0), 8)
    g2i.buffer('grid').set(q, grid)
    g2i.buffer('kernel1d').set(q, k1d)
    g2i.buffer('image').zero(q)
    g2i.set_w(w)
    g2i()
    img = g2i.buffer('image').get(q)
    full = np.zeros((P, G, G), np.complex128)
    gi.middle(full, grid.shape)[:] = grid
    want = grid_to_image_truth(full, k1d, lm_scale, lm_bias, w)
    assert tapered_relerr(img, want, k1d) <= 1e-12
    err = _peak_err(img, want)
    assert err <= 1e-12, 'grid->image: %.3g of the peak' % err
    # image -> grid from the image just made: against numpy, and the round trip against numpy's
    i2g.set_w(w)
    i2g()
    back = i2g.buffer('grid').get(q)
    want_back = image_to_grid_truth(want, k1d, lm_scale, lm_bias, w, Gg)
    assert _peak_err(back, want_back) <= 1e-12


@pytest.mark.gpu
def test_image_plane_ops_f64_exact():
    from katsdpimager_amd import image
    ctx, q = context_queue()
    P, H = 3, 40
    rs = np.random.RandomState(6)
    data = rs.standard_normal((P, H, H))
    sc = image.ScaleTemplate(ctx, np.float64, P).instantiate(q, (P, H, H))
    sc.ensure_all_bound()
    sc.buffer('data').set(q, data)
    factors = np.array([1 / 3, np.pi, -2.0 ** -40])
    sc.set_scale_factor(factors)
    sc()
    assert np.array_equal(sc.buffer('data').get(q), data * factors[:, None, None])
    ad = image.AddImageTemplate(ctx, np.float64, P).instantiate(q, (P, H, H))
    ad.ensure_all_bound()
    src = rs.standard_normal((P, H, H)) * 1e-9
    ad.buffer('src').set(q, src)
    ad.buffer('dest').set(q, data)
    ad()
    assert np.array_equal(ad.buffer('dest').get(q), data + src)
    pb = image.ApplyPrimaryBeamTemplate(ctx, np.float64, P).instantiate(q, (P, H, H), 0.3, np.nan)
    pb.ensure_all_bound()
    beam = rs.uniform(0, 1, (H, H))
    pb.buffer('data').set(q, data)
    pb.buffer('beam_power').set(q, beam)
    pb()
    want = np.where(beam < 0.3, np.nan, data / beam)
    np.testing.assert_array_equal(pb.buffer('data').get(q), want)


# ---------------------------------------------------------------------------------------------
# GPU: end to end through the operator classes

def _params(P, dtype, G=256):
    from katsdpimager_amd import parameters
    c = gi.make_config(G, 0.0001, 0.01, P, 28, 32, grid_cover=180, n_vis=3000)
    fixed_i = parameters.FixedImageParameters(list(range(P)), dtype)
    ip = parameters.ImageParameters(fixed_i, q_fov=1.0, image_oversample=None,
                                    wavelength=c['wavelength'], array=None,
                                    pixel_size=c['pixel_size'], pixels=c['pixels'])
    fixed_g = parameters.FixedGridParameters(c['antialias_width'], c['oversample'],
                                             c['image_oversample'], c['max_w'], c['kernel_width'])
    gp = parameters.GridParameters(fixed_g, c['w_slices'], c['w_planes'])
    ap = parameters.ArrayParameters(13.5, ip.cell_size * (c['grid_cover'] // 2))
    return c, ip, gp, ap


def _dirty(dtype, c, ip, gp, ap, t, wg_inner, w):
    from katsdpimager_amd import grid, image
    ctx, q = context_queue()
    fn = grid.GridderTemplate(ctx, ip.fixed, gp.fixed).instantiate(q, ap, ip, gp, 4096)
    fn.ensure_all_bound()
    n = len(t['uv'])
    wg = np.zeros(fn.buffer('grid').shape, np.float32)
    gi.middle(wg, wg_inner.shape)[:] = wg_inner
    fn.buffer('grid').zero(q)
    fn.buffer('weights_grid').set(q, wg)
    fn.num_vis = n
    fn.buffer('uv').set_region(q, t['uv'], np.s_[:n], np.s_[:])
    fn.buffer('w_plane').set_region(q, t['w_plane'], np.s_[:n], np.s_[:])
    fn.buffer('vis').set_region(q, t['vis'], np.s_[:n], np.s_[:])
    fn()
    G = ip.pixels
    tmpl = image.GridImageTemplate(ctx, dtype)
    g2i = tmpl.instantiate_grid_to_image(q, fn.buffer('grid').shape, ip.pixel_size,
                                         -0.5 * G * ip.pixel_size, tmpl.make_fft_plan((G, G)))
    g2i.bind(grid=fn.buffer('grid'))
    g2i.ensure_all_bound()
    k1d = fn.convolve_kernel.taper(G)
    g2i.buffer('kernel1d').set(q, k1d.astype(dtype))
    g2i.buffer('image').zero(q)
    g2i.set_w(w)
    g2i()
    return (g2i.buffer('image').get(q), fn.buffer('grid').get(q), fn.convolve_kernel.data, k1d,
            wg, fn.last_variant)


@pytest.mark.gpu
@pytest.mark.parametrize('w', [0.0, 3.0])
def test_point_source_dirty_image_f64(w):
    """A point source's dirty image from Gridder(float64) -> GridToImage(float64) against the
    float64 truth of the same pipeline (the contract's gridder, then GridToImageHost's formulas in
    float64), at 1e-11 of the taper-weighted peak; the float32 operators on the same data are at
    least 1e-8 away."""
    P = 2
    c, ip, gp, ap = _params(P, np.float64)
    rs = np.random.RandomState(8)
    t = gi.grid_track(c)
    n = c['n_vis']
    uvq = np.concatenate((t['uv'], t['sub_uv']), axis=1)
    # a point source at (l, m) = (3, -5) pixels: vis = exp(-2 pi i (l u + m v)) at the cell centres
    u = (t['uv'][:, 0] * c['oversample'] + t['sub_uv'][:, 0] + 0.5) / c['oversample']
    v = (t['uv'][:, 1] * c['oversample'] + t['sub_uv'][:, 1] + 0.5) / c['oversample']
    G = c['pixels']
    ph = np.exp(-2j * np.pi * (3 * u - 5 * v) / G)
    vis = np.stack([ph, 0.5 * ph], axis=1).astype(np.complex64)
    wg_inner = rs.uniform(0.5, 1.5, (P, c['grid_cover'], c['grid_cover'])).astype(np.float32)
    tt = dict(uv=uvq, w_plane=t['w_plane'], vis=vis)
    img, grid64, kern, k1d, wg, variant = _dirty(np.float64, c, ip, gp, ap, tt, wg_inner, w)
    assert variant == 'mfma' and grid64.dtype == np.complex128 and img.dtype == np.float64
    g_truth = grid_truth64(kern, uvq, t['w_plane'], vis, wg)
    assert _peak_err(grid64, g_truth) <= 1e-12
    full = np.zeros((P, G, G), np.complex128)
    gi.middle(full, g_truth.shape)[:] = g_truth
    want = grid_to_image_truth(full, k1d, ip.pixel_size, -0.5 * G * ip.pixel_size, w)
    assert tapered_relerr(img, want, k1d) <= 1e-11
    c32, ip32, gp32, ap32 = _params(P, np.float32)
    img32 = _dirty(np.float32, c32, ip32, gp32, ap32, tt, wg_inner, w)[0]
    assert tapered_relerr(img32, want, k1d) >= 1e-8
