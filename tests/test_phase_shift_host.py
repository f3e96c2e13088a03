"""Phase-centre shift without a device: the parameters object, the argument checks of
kimg_phase_shift (they run before any HIP call), the numpy twin (phaseshift.phase_shift_host, the
executable form of the contract in include/kimg.h) against visibilities synthesised directly in the
new frame, its composition with the uv-plane continuum fit, and the loader's keywords."""
import ctypes
import math

import numpy as np
import pytest

from katsdpimager_amd import continuum, loader, phaseshift
from katsdpimager_amd.phaseshift import PhaseShiftParameters, phase_shift_host, phase_shift_host_double

EINVAL = -10001
C0 = 299792458.0
O = (0.93, -0.52)               # the observation's phase centre (ra, dec), radians


def _direction(ra, dec):
    return np.array([math.cos(dec) * math.cos(ra), math.cos(dec) * math.sin(ra), math.sin(dec)])


def _lmn_minus_pole(centre, direction):
    """(l, m, n - 1) of a direction in a centre's frame, by the frame matrix (independent of the
    module's angle-difference forms), n - 1 without cancellation."""
    l, m, n = phaseshift.frame(*centre) @ _direction(*direction)
    return np.array([l, m, -(l * l + m * m) / (1.0 + n)])


def _source(uvw64, inv_wavelength, lmn1):
    """Unit source: exp(-2 pi i (l u + m v + (n - 1) w)), complex128 [C][N]."""
    turns = inv_wavelength[:, None] * (uvw64 @ lmn1)[None, :]
    return np.exp(-2j * np.pi * (turns - np.rint(turns)))


# ---- the parameters object --------------------------------------------------------------------------
@pytest.mark.parametrize('new', [(0.942, -0.515), (0.93 + 1e-5, -0.52), (0.93 - 2 * math.pi + 0.3, -0.9), (0.93, 0.4)])
def test_rotation_is_a_rotation_and_its_third_row_the_new_centre(new):
    p = PhaseShiftParameters(O, new)
    R = p.rotation
    assert np.abs(R @ R.T - np.identity(3)).max() <= 1e-15
    assert abs(np.linalg.det(R) - 1.0) <= 1e-15
    np.testing.assert_allclose(R[2], p.lmn, rtol=0, atol=1e-15)
    np.testing.assert_allclose(p.lmn, phaseshift.frame(*O) @ _direction(*new), rtol=0, atol=1e-15)
    np.testing.assert_allclose(p.delay[:2], p.lmn[:2], rtol=0, atol=0)
    back = PhaseShiftParameters(new, O)
    np.testing.assert_allclose(back.rotation, R.T, rtol=0, atol=1e-15)
    ra, dec = phaseshift.offset_to_radec(O, p.lmn[0], p.lmn[1])
    assert abs(math.remainder(ra - new[0], 2 * math.pi)) <= 1e-14 and abs(dec - new[1]) <= 1e-14


def test_equal_centres_give_the_identity_and_no_delay():
    p = PhaseShiftParameters(O, O)
    assert np.array_equal(p.rotation, np.identity(3))
    assert np.array_equal(p.delay, np.zeros(3)) and not p.writes_uvw
    assert np.array_equal(p.params12(), np.concatenate((np.identity(3).reshape(9), np.zeros(3))))
    assert PhaseShiftParameters(O, (0.94, -0.5)).writes_uvw
    # back to O from elsewhere: visibilities turn, coordinates do not
    q = PhaseShiftParameters(O, O, from_centre=(0.94, -0.5))
    assert np.array_equal(q.rotation, np.identity(3)) and not q.writes_uvw
    np.testing.assert_array_equal(q.delay, -PhaseShiftParameters(O, (0.94, -0.5)).delay)


def test_delay_keeps_its_digits_for_a_small_shift():
    """A shift of 1e-5 rad: n - 1 = -5e-11.  1 - n by subtraction in float64 is good to 1e-16 / 5e-11 =
    2e-6 of it; the stable form to rounding.  Truth in extended precision from the half-angle form
    n - 1 = -2 sin^2(dd / 2) - 2 cos dec' cos dec sin^2(da / 2)."""
    da, dd = np.longdouble(1e-5) * np.longdouble(0.6), np.longdouble(1e-5) * np.longdouble(0.8)
    new = (O[0] + float(da), O[1] + float(dd))
    da, dd = np.longdouble(new[0]) - np.longdouble(O[0]), np.longdouble(new[1]) - np.longdouble(O[1])
    truth = -2 * np.sin(dd / 2) ** 2 \
        - 2 * np.cos(np.longdouble(new[1])) * np.cos(np.longdouble(O[1])) * np.sin(da / 2) ** 2
    p = PhaseShiftParameters(O, new)
    assert abs(p.delay[2] / float(truth) - 1.0) <= 1e-10
    naive = float((phaseshift.frame(*O) @ _direction(*new))[2]) - 1.0
    assert abs(naive / float(truth) - 1.0) > 1e-8         # (what the stable form is there to avoid)
    assert -6e-11 < p.delay[2] < -2e-11


def test_parameters_refuse():
    for bad in (float('nan'), float('inf')):
        with pytest.raises(ValueError):
            PhaseShiftParameters((bad, 0.0), (0.1, 0.1))
        with pytest.raises(ValueError):
            PhaseShiftParameters((0.1, 0.1), (0.0, bad))
        with pytest.raises(ValueError):
            PhaseShiftParameters((0.1, 0.1), (0.1, 0.2), from_centre=(bad, 0.0))
    with pytest.raises(ValueError):
        PhaseShiftParameters((0.0, 0.0), (math.pi / 2 + 1e-9, 0.0))   # 90 degrees away
    with pytest.raises(ValueError):
        PhaseShiftParameters((0.0, 0.0), (2.0, 0.0))                  # further
    with pytest.raises(ValueError):
        PhaseShiftParameters((0.0, 0.3), (0.0, 0.3 - 1.6))
    with pytest.raises(ValueError):
        PhaseShiftParameters((0.0, 0.0), (0.1, 0.0), from_centre=(2.0, 0.0))
    with pytest.raises(ValueError):
        PhaseShiftParameters((0.0,), (0.1, 0.0))
    with pytest.raises(ValueError):
        PhaseShiftParameters(None, (0.1, 0.0))
    PhaseShiftParameters((0.0, 0.0), (1.57, 0.0))                     # just inside


# ---- refusals of the entry point --------------------------------------------------------------------
def test_entry_point_refuses_before_any_hip_call():
    from katsdpimager_amd import _lib
    fn = _lib.lib().kimg_phase_shift
    host = np.concatenate((np.identity(3).reshape(9), np.zeros(3)))
    base = 1 << 20                                      # (never dereferenced)

    def call(C=4, N=8, Q=2, pitch=16, vis=base, uvw_in=2 * base, uvw_out=3 * base, inv=4 * base,
             params=host):
        as_p = lambda x: None if x is None else ctypes.c_void_p(x)      # noqa: E731
        return fn(as_p(vis), pitch, C, N, Q, as_p(uvw_in), as_p(uvw_out), as_p(inv),
                  None if params is None else params.ctypes.data_as(ctypes.c_void_p), None)
    for null in ('vis', 'uvw_in', 'inv', 'params'):
        assert call(**{null: None}) == EINVAL
    assert call(C=0) == EINVAL
    assert call(C=-3) == EINVAL
    assert call(Q=0) == EINVAL
    assert call(N=-1) == EINVAL
    assert call(pitch=15) == EINVAL                     # channels would overlap
    # uvw arrays that overlap: the same, one float apart, the last row on the first
    assert call(uvw_out=2 * base) == EINVAL
    assert call(uvw_out=2 * base + 4) == EINVAL
    assert call(uvw_out=2 * base + 8 * 12 - 4) == EINVAL
    assert call(uvw_out=2 * base - 8 * 12 + 4) == EINVAL
    # nothing to do, nothing launched (and nothing dereferenced): adjoining arrays are fine
    assert call(N=0, pitch=0) == 0
    assert call(N=0, pitch=0, uvw_out=None) == 0
    assert call(N=0, pitch=0, uvw_out=2 * base) == 0


# ---- the twin ---------------------------------------------------------------------------------------
def _geometry(seed=3, N=400, C=6):
    rng = np.random.default_rng(seed)
    uvw = rng.uniform(-1.0, 1.0, (N, 3))
    uvw *= (8000.0 * rng.uniform(0.01, 1.0, N) / np.linalg.norm(uvw, axis=1))[:, None]
    uvw = uvw.astype(np.float32)                                # baselines to 8 km
    freq = 1.4e9 + 1.0e6 * np.cumsum(rng.uniform(0.2, 1.7, C))  # non-uniform
    return uvw, freq / C0


T = (0.93 + 0.011, -0.52 + 0.0075)       # about 0.7 degrees from O
S2 = (0.93 - 0.004, -0.52 + 0.013)       # an arbitrary second source


def test_twin_puts_a_source_at_the_new_centre_on_one():
    uvw, inv_wl = _geometry()
    x = uvw.astype(np.float64)
    p = PhaseShiftParameters(O, T)
    truth = _source(x, inv_wl, _lmn_minus_pole(O, T))
    assert np.abs(inv_wl[:, None] * (x @ p.delay)[None]).max() > 300       # hundreds of turns
    vis = np.repeat(truth[:, :, None], 2, axis=2).astype(np.complex64)
    out, new_uvw = phase_shift_host_double(vis, uvw, inv_wl, p)
    # the input's rounding to complex64 (2^-24 per component of a unit value) and nothing else
    assert np.abs(out - 1.0).max() <= math.sqrt(2.0) * 2.0 ** -24 + 1e-9
    # against the unrounded input: the rotation itself is good to 1e-9
    assert np.abs(out[:, :, 0] - vis[:, :, 0].astype(np.complex128) / truth).max() <= 1e-9
    rounded, uvw32 = phase_shift_host(vis, uvw, inv_wl, p)
    assert rounded.dtype == np.complex64 and uvw32.dtype == np.float32
    np.testing.assert_array_equal(rounded, out.astype(np.complex64))
    np.testing.assert_array_equal(uvw32, new_uvw.astype(np.float32))
    # w' - w is the delay in metres; lengths are kept
    np.testing.assert_allclose(new_uvw[:, 2] - x[:, 2], x @ p.delay, rtol=0, atol=1e-11)
    np.testing.assert_allclose(np.linalg.norm(new_uvw, axis=1), np.linalg.norm(x, axis=1), rtol=1e-14)


def test_twin_moves_any_source_into_the_new_frame():
    """A second source, synthesised in the frame of O from the float32 coordinates, comes out as its
    visibilities synthesised in the frame of T from the float64 uvw' (the input's complex64 rounding
    carried along as the factor it is)."""
    uvw, inv_wl = _geometry(seed=4)
    x = uvw.astype(np.float64)
    p = PhaseShiftParameters(O, T)
    old = 0.7 * _source(x, inv_wl, _lmn_minus_pole(O, S2))
    vis = old[:, :, None].astype(np.complex64)
    out, new_uvw = phase_shift_host_double(vis, uvw, inv_wl, p)
    new = 0.7 * _source(new_uvw, inv_wl, _lmn_minus_pole(T, S2))
    carried = vis[:, :, 0].astype(np.complex128) / old
    assert np.abs(carried - 1.0).max() <= 2.0 ** -23
    assert np.abs(out[:, :, 0] - new * carried).max() <= 1e-9
    assert np.abs(out[:, :, 0] - new).max() <= 2.0 ** -23          # and so to the input's rounding


def test_two_steps_through_from_centre_equal_one():
    uvw, inv_wl = _geometry(seed=5)
    ones = np.ones((len(inv_wl), len(uvw), 1), np.complex64)
    direct, direct_uvw = phase_shift_host_double(ones, uvw, inv_wl, PhaseShiftParameters(O, T))
    first, _ = phase_shift_host_double(ones, uvw, inv_wl, PhaseShiftParameters(O, S2))
    second, second_uvw = phase_shift_host_double(ones, uvw, inv_wl,
                                                 PhaseShiftParameters(O, T, from_centre=S2))
    assert np.abs(first * second - direct).max() <= 1e-9
    np.testing.assert_array_equal(second_uvw, direct_uvw)
    # and there and back again is nothing
    back, _ = phase_shift_host_double(ones, uvw, inv_wl, PhaseShiftParameters(O, O, from_centre=T))
    assert np.abs(direct * back - 1.0).max() <= 1e-9


def test_non_finite_inputs_stay_in_their_sample():
    uvw, inv_wl = _geometry(seed=6, N=12, C=3)
    rng = np.random.default_rng(1)
    vis = (rng.normal(size=(3, 12, 2)) + 1j * rng.normal(size=(3, 12, 2))).astype(np.complex64)
    uvw[2, 1] = np.nan
    uvw[7, 0] = np.inf
    vis[1, 4, 0] = complex(np.nan, 1.0)
    vis[2, 9, 1] = complex(2.0, -np.inf)
    out, new_uvw = phase_shift_host(vis, uvw, inv_wl, PhaseShiftParameters(O, T))
    bad = np.zeros(vis.shape, bool)
    bad[:, [2, 7], :] = True
    bad[1, 4, 0] = bad[2, 9, 1] = True
    assert np.array_equal(~np.isfinite(out.real), bad) and np.array_equal(~np.isfinite(out.imag), bad)
    assert np.array_equal(~np.isfinite(new_uvw), np.isin(np.arange(12), [2, 7])[:, None].repeat(3, 1))


# ---- with the continuum fit -------------------------------------------------------------------------
def test_continuum_fit_on_the_source_instead_of_the_phase_centre():
    """A 2 Jy continuum source with spectral index -0.7, 0.6 / 0.3 degrees off centre, 32 channels
    over 1.40-1.43 GHz, baselines to 4 km, order 1, eight line channels left out of the fit, through
    the twins only: the largest residual over all channels with the fit on the source is at least
    1000 times below the one with the fit around the phase centre."""
    rng = np.random.default_rng(8)
    N, C = 300, 32
    uvw = rng.uniform(-1.0, 1.0, (N, 3))
    uvw *= (4000.0 * rng.uniform(0.05, 1.0, N) / np.linalg.norm(uvw, axis=1))[:, None]
    uvw = uvw.astype(np.float32)
    freq = np.linspace(1.40e9, 1.43e9, C)
    inv_wl = freq / C0
    source = (O[0] + math.radians(0.6) / math.cos(O[1]), O[1] + math.radians(0.3))
    flux = 2.0 * (freq / freq[0]) ** -0.7
    vis = (flux[:, None] * _source(uvw.astype(np.float64), inv_wl, _lmn_minus_pole(O, source)))
    vis = vis[:, :, None].astype(np.complex64)
    weights = np.ones(vis.shape, np.float32)
    params = continuum.UVContSubParameters(1, line_ranges=[(12, 20)], frequencies=freq)
    plain, _, counts = continuum.uvcontsub_host(vis, weights, params)
    assert counts == (N, 0)
    there, _ = phase_shift_host(vis, uvw, inv_wl, PhaseShiftParameters(O, source))
    fitted, _, _ = continuum.uvcontsub_host(there, weights, params)
    back, same_uvw = phase_shift_host(fitted, uvw, inv_wl, PhaseShiftParameters(O, O, from_centre=source))
    np.testing.assert_array_equal(same_uvw, uvw)
    without, with_centre = float(np.abs(plain).max()), float(np.abs(back).max())
    print('largest residual: around the phase centre {:.3g}, on the source {:.3g}'.format(
        without, with_centre))
    assert without > 1.0                    # (the fit around the phase centre is no use here)
    assert with_centre * 1000.0 <= without


# ---- the loader's keywords --------------------------------------------------------------------------
class _Recorder:
    queue = None

    def __init__(self):
        self.calls = []

    def add(self, *args):
        self.calls.append(('add',) + args)

    def close(self):
        self.calls.append(('close',))


def _dataset(rows=50, C=3):
    rng = np.random.default_rng(2)
    vis = (rng.normal(size=(rows, C, 1)) + 1j * rng.normal(size=(rows, C, 1))).astype(np.complex64)
    return loader.LoaderArrays(rng.normal(size=(rows, 3)).astype(np.float32), vis,
                               np.ones((rows, C, 1), np.float32), np.arange(rows) % 7,
                               1.4e9 + 1e6 * np.arange(C), [0], phase_centre=O)


def test_continuum_centre_needs_continuum():
    rec = _Recorder()
    with pytest.raises(ValueError):
        loader.preprocess_visibilities(_dataset(), rec, 0, 3, (np.identity(1), None),
                                       continuum_centre=T)
    with pytest.raises(ValueError):
        loader.preprocess_visibilities(_dataset(), rec, 0, 3, (np.identity(1), None),
                                       phase_centre=T, continuum_centre=S2)


def test_without_the_keywords_the_collector_sees_what_it_saw():
    ds = _dataset()
    ident = np.identity(1, np.complex64)
    rec = _Recorder()
    assert loader.preprocess_visibilities(ds, rec, 0, 3, (ident, None), vis_load=3 * 20,
                                          phase_centre=None, continuum_centre=None) is rec
    chunks = list(loader.data_iter(ds, None, 3 * 20, 0, 3))
    assert len(chunks) == 3 and len(rec.calls) == 4 and rec.calls[-1] == ('close',)
    for call, chunk in zip(rec.calls, chunks):
        assert call[0] == 'add' and len(call) == 8
        for got, key in zip(call[1:4], ('uvw', 'weights', 'vis')):
            assert type(got) is np.ndarray and got.dtype == chunk[key].dtype
            np.testing.assert_array_equal(got, chunk[key])
        assert call[4] is None and call[5] is None and call[6] is ident and call[7] is None
    assert not hasattr(rec, 'phase_centre') and not hasattr(rec, 'continuum_counts')
