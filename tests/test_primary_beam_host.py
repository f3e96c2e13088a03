"""Primary-beam correction without a GPU: the beam model (RadialBeam), the numpy statement of the
device contract (sample_host, correct_host) against the reference's sampler restated in float64,
the C ABI surface of kimg_primary_beam and its refusals, and the driver's keyword."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from katsdpimager_amd import primary_beam as pb
from katsdpimager_amd.primary_beam import RadialBeam, PrimaryBeamParameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIMG_EINVAL = -10001
EPS32 = 2.0 ** -24              # half an ulp of 1: the relative error of one float32 rounding


def table():
    rs = np.random.RandomState(3)
    samples = rs.uniform(-1.0, 1.0, (3, 7))
    return RadialBeam(0.01, [1.0e9, 1.5e9, 1.75e9], samples, band='L')


def test_row_interpolates_in_frequency():
    """The table row itself at a tabulated frequency, the float64 lerp rounded once in between,
    NaN -- no error -- below and above the range (the reference's test_out_of_range)."""
    beam = table()
    for i, f in enumerate(beam.frequencies):
        row = beam.row(f)
        assert row.dtype == np.float32 and row.shape == (7,)
        np.testing.assert_array_equal(row, beam.samples[i].astype(np.float32))
    a, b = beam.samples[1], beam.samples[2]
    np.testing.assert_array_equal(beam.row(1.625e9), (a * 0.5 + b * 0.5).astype(np.float32))
    t = (1.2e9 - 1.0e9) / (1.5e9 - 1.0e9)
    np.testing.assert_array_equal(beam.row(1.2e9),
                                  (beam.samples[0] * (1.0 - t) + beam.samples[1] * t).astype(np.float32))
    for f in (0.999e9, 1.7500001e9, 0.0, np.nan):
        row = beam.row(f)
        assert row.dtype == np.float32 and row.shape == (7,) and np.all(np.isnan(row))
    assert beam.frequency_range() == (1.0e9, 1.75e9)
    assert beam.inradius() == pytest.approx(0.06)
    float32_table = RadialBeam(0.01, [1e9], beam.samples[:1].astype(np.float32))
    np.testing.assert_array_equal(float32_table.row(1e9), float32_table.samples[0])


def test_radial_beam_refuses_bad_tables():
    with pytest.raises(ValueError):
        RadialBeam(0.01, [1e9], np.ones(5))                 # not 2-D
    with pytest.raises(ValueError):
        RadialBeam(0.01, [1e9], np.ones((1, 1)))            # one radial sample
    with pytest.raises(ValueError):
        RadialBeam(0.01, [1e9, 2e9], np.ones((3, 4)))       # rows and frequencies differ
    with pytest.raises(ValueError):
        RadialBeam(0.01, [2e9, 1e9], np.ones((2, 4)))       # not increasing
    with pytest.raises(ValueError):
        RadialBeam(0.0, [1e9], np.ones((1, 4)))


FWHM = 0.02
STEP = 1.0e-4


def cosine():
    return RadialBeam.cosine_taper(FWHM, 1.0e9, [0.8e9, 1.0e9, 2.0e9], STEP, 0.05)


def test_cosine_taper_centre_and_half_power():
    """Power 1 at the centre (a table entry) and 1/2 at fwhm / 2, which lies between two entries
    whenever the frequency scaling puts it there: linear interpolation of V over an interval h is
    off by at most h^2 max|V''| / 8, and |V''| <= (c / fwhm)^2 max|d2V/dr2| with
    |d2V/dr2| <= pi^2 - 8 for the cosine taper (from V = 1 - (pi^2 / 2 - 4) r^2 + ...: its value at
    r = 0, where it is largest).  The power's error is at most 2 |V| <= 2 times that plus its
    square."""
    beam = cosine()
    c = 2.0 * pb._cosine_taper_half_power()
    assert 1.18 < c < 1.20          # (the known 1.189 of the cosine taper)
    for f in beam.frequencies:
        width = FWHM * 1.0e9 / f
        row = beam.row(f).astype(np.float64)
        assert row[0] == 1.0
        s = 0.5 * width / STEP
        pos = int(s)
        v = row[pos] + (row[pos + 1] - row[pos]) * (s - pos)
        second = (c / width) ** 2 * (np.pi ** 2 - 8.0)
        tol_v = STEP ** 2 * second / 8.0 + 2.0 * EPS32       # (+ the float32 rounding of the row)
        assert abs(v * v - 0.5) <= 2.0 * tol_v + tol_v ** 2
        assert abs(v * v - 0.5) > 0 or s == pos


def test_cosine_taper_singularity_is_finite():
    """r = 1/2 exactly: fwhm(nu) = c * rho there.  V = pi / 4."""
    assert pb._cosine_taper_voltage(0.5) == pytest.approx(np.pi / 4.0, rel=1e-15)
    near = pb._cosine_taper_voltage(np.array([0.5 - 1e-9, 0.5 + 1e-9]))
    np.testing.assert_allclose(near, np.pi / 4.0, rtol=1e-8)
    # against the textbook form away from the singularity
    r = np.array([0.0, 0.1, 0.49, 0.51, 0.9, 1.5, 2.2])
    np.testing.assert_allclose(pb._cosine_taper_voltage(r), np.cos(np.pi * r) / (1.0 - 4.0 * r * r),
                               rtol=1e-12, atol=1e-15)
    c = 2.0 * pb._cosine_taper_half_power()
    beam = RadialBeam.cosine_taper(2.0 * c * 0.01, 1.0e9, [1.0e9], 0.01, 0.05)     # rho = 0.01: r = 1/2
    assert np.all(np.isfinite(beam.samples))
    assert beam.samples[0][1] == pytest.approx(np.pi / 4.0, rel=1e-12)


def test_cosine_taper_scales_with_frequency():
    """The pattern at 2 nu at radius rho is the pattern at nu at 2 rho."""
    beam = cosine()
    np.testing.assert_allclose(beam.samples[2][:200], beam.samples[1][:400:2], rtol=1e-12, atol=1e-15)
    assert beam.samples.shape == (3, 501)


def test_save_load_round_trip(tmp_path):
    beam = cosine()
    name = str(tmp_path / 'beam.npz')
    beam.save(name)
    back = RadialBeam.load(name)
    assert back == beam and hash(back) == hash(beam) and back.band is None
    np.testing.assert_array_equal(back.samples, beam.samples)
    np.testing.assert_array_equal(back.frequencies, beam.frequencies)
    assert back.step == beam.step
    named = table()
    named.save(name)
    assert RadialBeam.load(name).band == 'L' and RadialBeam.load(name) != beam


def test_parameters_hash_compare_repr():
    a = PrimaryBeamParameters(cosine())
    b = PrimaryBeamParameters(cosine(), cutoff=0.1)
    c = PrimaryBeamParameters(cosine(), cutoff=0.2)
    assert a == b and hash(a) == hash(b) and a != c and a.cutoff == 0.1
    assert len({a, b, c}) == 2
    assert 'PrimaryBeamParameters' in repr(a) and 'cutoff=0.1' in repr(a)
    with pytest.raises(TypeError):
        PrimaryBeamParameters(np.ones((2, 3)))
    with pytest.raises(ValueError):
        PrimaryBeamParameters(cosine(), cutoff=np.nan)


# The reference test's geometry: 101 x 101 pixels 0.001 apart, centred.  The table's step is not
# commensurate with the pixels, and its last sample lies between the edge (0.05) and the corner
# (0.0707) of the grid, so that both the interpolated region and the NaN region are there.
N = 101
PIXEL = 0.001
TABLE_STEP = 0.00037
TABLE_R = 163


def test_sample_host_against_float64():
    """sample_host (float32, multiplies by float32(1 / step)) against sample_float64 (the
    reference's sampler in float64).  With u = 2^-24, L = 0.05 the largest |coordinate|, S the
    largest s that is interpolated (< R - 1), D = max |row[i + 1] - row[i]| and V = max |row|:
      l, m:    float32(scale) (u), the product (u, of at most 2 L), float32(bias) (u L) and the sum
               (u L): at most 6 L u absolute each
      radius:  sqrt(dl^2 + dm^2) <= 6 sqrt(2) L u from the coordinates, 2 u radius <= 2 sqrt(2) L u
               from the two squares, the sum and the root (the root halves the first three):
               8 sqrt(2) L u, which is 8 S_max u in units of the step, S_max the corner's s
      s:       inv_step (u) and the product (u): 2 u s more.  ds <= (8 S_max + 2 S) u
      v:       the interpolant is continuous and piecewise linear with slope at most D per unit
               of s, so a shifted s moves it by at most D ds whether or not pos changes; the
               difference (u D), its product with frac < 1 (u D) and the sum (u V) add
               (2 D + V) u
      power:   2 V dv + dv^2 + u V^2
    Pixels whose float64 s lies within 1e-3 of R - 1 are left out (only there may the NaN
    decision differ): they must be at most 0.5 % of the grid."""
    beam = RadialBeam.cosine_taper(0.05, 1.0e9, [1.0e9], TABLE_STEP, TABLE_STEP * (TABLE_R - 1))
    assert beam.samples.shape[1] == TABLE_R
    row = beam.row(1.0e9)
    bias = -(N // 2) * PIXEL
    got = pb.sample_host(row, TABLE_STEP, N, N, PIXEL, bias)
    want = pb.sample_float64(row, TABLE_STEP, N, N, PIXEL, bias)
    assert got.dtype == np.float32 and got.shape == want.shape == (N, N)
    coords = np.arange(N) * PIXEL + bias
    s64 = np.hypot(coords[None, :], coords[:, None]) / TABLE_STEP
    left_out = np.abs(s64 - (TABLE_R - 1)) < 1e-3
    assert left_out.sum() <= 0.005 * N * N
    use = ~left_out
    np.testing.assert_array_equal(np.isnan(got)[use], np.isnan(want)[use])
    assert 0.05 < np.isnan(want).mean() < 0.5          # both regions are there
    assert got[N // 2, N // 2] == 1.0                   # s = 0 exactly: the first sample
    u = EPS32
    L = 0.05
    s_max = np.sqrt(2.0) * L / TABLE_STEP
    S = TABLE_R - 1
    D = float(np.max(np.abs(np.diff(row.astype(np.float64)))))
    V = float(np.max(np.abs(row)))
    ds = (8.0 * s_max + 2.0 * S) * u
    dv = D * ds + (2.0 * D + V) * u
    bound = 2.0 * V * dv + dv * dv + u * V * V
    finite = use & ~np.isnan(want)
    measured = float(np.max(np.abs(got[finite].astype(np.float64) - want[finite])))
    print('sample_host vs float64: measured {:.3e}, bound {:.3e}'.format(measured, bound))
    assert bound < 5e-6
    assert measured <= bound


def test_sample_host_rectangular_and_tiny_table():
    """Width and height are separate; R = 2 interpolates inside the first interval only."""
    row = np.array([1.0, 0.5], np.float32)
    got = pb.sample_host(row, 0.25, 5, 3, 0.1, -0.2)
    assert got.shape == (3, 5)
    l = np.arange(5, dtype=np.float32) * np.float32(0.1) + np.float32(-0.2)
    m = np.arange(3, dtype=np.float32) * np.float32(0.1) + np.float32(-0.2)
    for y in range(3):
        for x in range(5):
            s = np.float32(np.sqrt(np.float32(l[x] * l[x]) + np.float32(m[y] * m[y]))) * np.float32(4.0)
            if s < 1:
                v = np.float32(1.0) + np.float32(np.float32(-0.5) * s)
                assert got[y, x] == np.float32(v * v)
            else:
                assert np.isnan(got[y, x])
    assert np.isnan(got).any() and not np.isnan(got).all()


def test_correct_host_threshold_and_nan():
    power = np.array([[0.25, 0.5, np.nan, 0.1]], np.float32)
    model = np.array([[[1.0, 2.0, 3.0, 4.0]], [[5.0, 6.0, 7.0, 8.0]]], np.float32)
    dirty = model + np.float32(10)
    want_dirty = dirty.copy()
    keep = pb.correct_host(power, model, dirty, 0.25)
    np.testing.assert_array_equal(keep, [[True, True, False, False]])       # power == threshold stays
    np.testing.assert_array_equal(model, np.array([[[4.0, 4.0, 0.0, 0.0]], [[20.0, 12.0, 0.0, 0.0]]],
                                                  np.float32))
    assert np.all(np.isnan(dirty[:, :, 2:])) and not np.any(np.isnan(dirty[:, :, :2]))
    np.testing.assert_array_equal(dirty[:, :, :2], want_dirty[:, :, :2] / power[:, :2])
    assert model.dtype == dirty.dtype == np.float32


def test_header_export_and_prototype():
    from katsdpimager_amd import _lib, build
    header = open(os.path.join(ROOT, 'include', 'kimg.h')).read()
    assert re.search(r'\bint\s+kimg_primary_beam\s*\(', header)
    assert re.search(r'#define KIMG_VERSION 5\b', header)
    limit = int(re.search(r'#define KIMG_PRIMARY_BEAM_MAX_SAMPLES (\d+)', header).group(1))
    assert limit == _lib.PRIMARY_BEAM_MAX_SAMPLES >= 1024
    assert 'primary_beam.hip' in build.SOURCES
    restype, argtypes = _lib.PROTOTYPES['kimg_primary_beam']
    assert restype is ctypes.c_int and len(argtypes) == 16
    build.build_lib()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), 'kimg_primary_beam')
    declaration = re.search(r'int\s+kimg_primary_beam\s*\(([^;]*)\)\s*;', header).group(1)
    assert '_stride' not in declaration and declaration.count('_pitch') == 3


def test_refusals_without_gpu():
    """Every bad argument is KIMG_EINVAL before any HIP call (there is no device here)."""
    from katsdpimager_amd import _lib
    lib = _lib.lib()
    one = ctypes.c_void_p(64)
    two = ctypes.c_void_p(128)
    good = dict(beam=one, beam_pitch=8, model=one, dirty=two, row_pitch=8, pol_pitch=64, width=8,
                height=8, pols=2, row=one, samples=16, inv_step=100.0, scale=0.01, bias=-0.04,
                threshold=0.1)

    def call(**change):
        a = dict(good, **change)
        return lib.kimg_primary_beam(a['beam'], a['beam_pitch'], a['model'], a['dirty'], a['row_pitch'],
                                     a['pol_pitch'], a['width'], a['height'], a['pols'], a['row'],
                                     a['samples'], a['inv_step'], a['scale'], a['bias'], a['threshold'],
                                     None)
    bad = [dict(row=None), dict(width=0), dict(width=-3), dict(height=0), dict(height=-1),
           dict(pols=0), dict(pols=5), dict(pols=-1),
           dict(samples=1), dict(samples=0), dict(samples=-2),
           dict(samples=_lib.PRIMARY_BEAM_MAX_SAMPLES + 1),
           dict(model=None), dict(dirty=None),                      # one image without the other
           dict(model=None, dirty=None, beam=None),                 # nothing to do
           dict(model=None, dirty=None, pols=0),                    # P is checked without images too
           dict(beam_pitch=7), dict(row_pitch=7), dict(row_pitch=-8), dict(pol_pitch=63),
           dict(pol_pitch=-64), dict(dirty=one),                    # the two images are one
           dict(inv_step=0.0), dict(inv_step=-1.0), dict(inv_step=float('nan'))]
    for change in bad:
        assert call(**change) == KIMG_EINVAL, change


def test_process_channel_signature():
    from katsdpimager_amd import frontend, imaging
    params = list(inspect.signature(frontend.process_channel).parameters.values())
    names = [p.name for p in params]
    assert 'primary_beam' in names
    assert params[names.index('primary_beam')].default is None
    assert names[-1] == 'auto_mask' and names[-2] == 'primary_beam'
    assert callable(imaging.Imaging.primary_beam_correct)
    assert callable(pb.PrimaryBeamTemplate)
