"""The stopping threshold of a major cycle's minor cycles, to the last bit, on every route.

The contract (include/kimg.h, kimg_clean_major_cycles; frontend.py:560-575 of the reference) is
restated once, in float64, by :func:`expected_threshold`.  The host tests drive
``frontend.process_channel`` with recorder imagers and hold the numbers it hands on against that
restatement; the device tests build images whose outcome flips with one float32 ulp of threshold
and run them through every form of the loop and through the driver's three routes, against the
restated CleanHost (oracle/kimg_oracle.Clean) stopped at the restatement's threshold.  Every
comparison is exact."""
import functools
import math

import numpy as np
import pytest

from oracle import kimg_oracle as orc
from test_host_logic import _HostReader, _Recorder, _ShortCutRecorder, _driver_params

gpu = pytest.mark.gpu

CLEAN_I, CLEAN_SUMSQ = 0, 1
F = np.float32


@functools.lru_cache(maxsize=None)
def _scale(mode, sigma, P):
    """clean.noise_threshold_scale, computed once per argument set (SciPy's tails are slow)."""
    from katsdpimager_amd import clean
    return clean.noise_threshold_scale(mode, sigma, P)


def expected_threshold(mode, P, first_metric_f32, noise_f32, sigma, major_gain):
    """(stop after the first cycle, threshold of the later cycles as the float32 metric they are
    compared with): every operation in float64, one rounding to float32 at the end."""
    from katsdpimager_amd import clean
    metric = float(F(first_metric_f32))
    power = clean.metric_to_power(mode, metric)
    noise_threshold = float(noise_f32) * _scale(mode, sigma, P)
    left = 1.0 - major_gain
    T = max(float(noise_threshold), left * power)
    return bool(power <= T), F(clean.power_to_metric(mode, T))


def float32_threshold(mode, P, first_metric_f32, noise_f32, sigma, major_gain):
    """The same expression with every operation rounded to float32 (what a float32 scalar next to a
    Python float computes under NumPy 2): what the threshold must NOT be."""
    from katsdpimager_amd import clean
    power = F(first_metric_f32) if mode == CLEAN_I else np.sqrt(F(first_metric_f32))
    T = max(F(noise_f32) * F(_scale(mode, sigma, P)),
            F(1.0 - major_gain) * power)
    return F(T) if mode == CLEAN_I else F(T * T)


def test_expected_threshold_known_values():
    """The restatement on values worked out by hand (all exact in binary)."""
    # CLEAN_I: the major gain decides: 0.25 x 6 = 1.5; the noise decides: 0.5 x 4 = 2
    assert expected_threshold(CLEAN_I, 1, F(6.0), F(0.25), 4.0, 0.75) == (False, F(1.5))
    assert expected_threshold(CLEAN_I, 1, F(6.0), F(0.5), 4.0, 0.75) == (False, F(2.0))
    # ... a peak that is not above the threshold, with equality and one ulp of the noise below it
    assert expected_threshold(CLEAN_I, 1, F(6.0), F(1.5), 4.0, 0.75) == (True, F(6.0))
    stop, t = expected_threshold(CLEAN_I, 1, F(6.0), np.nextafter(F(1.5), F(0)), 4.0, 0.75)
    assert (stop, t) == (False, np.nextafter(F(6.0), F(0)))
    # CLEAN_SUMSQ: metric 16 is a flux of 4; 0.25 x 4 = 1, squared
    assert expected_threshold(CLEAN_SUMSQ, 3, F(16.0), F(0.0), 5.0, 0.75) == (False, F(1.0))
    # one rounding, at the end: 0.15 x 3 in doubles, not float32(0.15) x 3
    stop, t = expected_threshold(CLEAN_I, 1, F(3.0), F(0.0), 5.0, 0.85)
    assert t == F((1.0 - 0.85) * 3.0) and t != F(1.0 - 0.85) * F(3.0)


# ---------------------------------------------------------------------------------------------
# the host's arithmetic (no device)

class _Float32Recorder(_Recorder):
    """_Recorder whose peak and noise estimate are float32 scalars, as Imaging's are, and which
    keeps the thresholds it is handed."""

    def __init__(self, num_pols, peak, noise):
        super().__init__(num_pols=num_pols, peaks=[F(peak)], cycles_before_threshold=2)
        self._noise = F(noise)
        self.thresholds = []

    def noise_est(self):
        self.calls.append(('noise_est',))
        return self._noise

    def clean_cycle(self, psf_patch, threshold=0.0):
        if threshold != 0.0:
            self.thresholds.append(threshold)
        return super().clean_cycle(psf_patch, threshold)

    def clean_cycles(self, psf_patch, threshold, max_cycles):
        self.thresholds.append(threshold)
        return super().clean_cycles(psf_patch, threshold, max_cycles)


class _Float32ShortCutRecorder(_ShortCutRecorder):
    def __init__(self, num_pols, peak, noise):
        # (the one call hands the first metric back as the C float it is: a Python float)
        super().__init__(num_pols=num_pols, peaks=[float(F(peak))], cycles_before_threshold=2)
        self._noise = F(noise)
        self.handed = []

    def noise_est(self):
        self.calls.append(('noise_est',))
        return self._noise

    def clean_major_cycles(self, psf_patch, noise_threshold, left_for_next, max_cycles, batcher=None):
        self.handed.append((noise_threshold, left_for_next))
        return super().clean_major_cycles(psf_patch, noise_threshold, left_for_next, max_cycles, batcher)


SIGMA = 4.7         # (5.0 x a float32 is exact in doubles: its float32 product could not differ)
HOST_CASES = 300


@functools.lru_cache(maxsize=None)
def _host_inputs(mode, P, major_gain):
    """Seeded (first metric, noise estimate) pairs, both float32: the major gain decides for most,
    the noise for some, and for some the first peak is not above the threshold at all."""
    from katsdpimager_amd import clean
    rs = np.random.RandomState(1000 * mode + 100 * P + int(round(1000 * major_gain)))
    scale = float(clean.noise_threshold_scale(mode, SIGMA, P))
    left = 1.0 - major_gain
    out = []
    for kind in rs.choice(['gain', 'noise', 'stop'], HOST_CASES, p=[0.6, 0.3, 0.1]):
        power = rs.uniform(0.5, 4.0)
        if kind == 'gain':
            target = left * power * rs.uniform(0.2, 0.9)
        elif kind == 'noise':
            target = power * (left + (1.0 - left) * rs.uniform(0.05, 0.9))
        else:
            target = power * rs.uniform(1.0, 1.5)
        out.append((F(clean.power_to_metric(mode, power)), F(target / scale)))
    want = [expected_threshold(mode, P, m, n, SIGMA, major_gain) for m, n in out]
    naive = [float32_threshold(mode, P, m, n, SIGMA, major_gain) for m, n in out]
    # the inputs can tell the two arithmetics apart, and every outcome occurs
    differ = sum(1 for (stop, t), u in zip(want, naive) if t != u)
    stops = sum(1 for stop, t in want if stop)
    noise_decides = sum(1 for (m, n), (stop, t) in zip(out, want)
                        if not stop and t == F(clean.power_to_metric(mode, float(n) * scale)))
    if mode == CLEAN_I and major_gain == 0.85:
        assert differ >= HOST_CASES // 4, differ
    assert differ >= HOST_CASES // 10, differ
    assert HOST_CASES // 20 <= stops <= HOST_CASES // 5, stops
    assert noise_decides >= HOST_CASES // 5 and HOST_CASES - stops - noise_decides >= HOST_CASES // 3
    return out, want


def _host_params(mode, P, major_gain, minor=10):
    image_p, grid_p, clean_p = _driver_params(major_gain=major_gain, threshold=SIGMA, minor=minor)
    image_p.fixed.polarizations = list(range(P))
    clean_p.mode = mode
    return image_p, grid_p, clean_p


HOST_MODES = [(CLEAN_I, 1), (CLEAN_SUMSQ, 1), (CLEAN_SUMSQ, 3)]


@pytest.mark.parametrize('batched', [True, False])
@pytest.mark.parametrize('major_gain', [0.85, 0.999, 0.3])
@pytest.mark.parametrize('mode,P', HOST_MODES)
def test_host_threshold_in_two_steps(mode, P, major_gain, batched):
    """The reference's two steps: the threshold that reaches clean_cycles / clean_cycle is the
    restatement's, bit for bit, and no further cycle runs exactly when it says so."""
    from katsdpimager_amd import frontend, weight
    inputs, want = _host_inputs(mode, P, major_gain)
    image_p, grid_p, clean_p = _host_params(mode, P, major_gain)
    for (metric, noise), (stop, threshold) in zip(inputs, want):
        im = _Float32Recorder(P, metric, noise)
        out = frontend.process_channel(_HostReader([1]), 0, im, image_p, grid_p, clean_p,
                                       weight.WeightType.NATURAL, 4, 1, True, batched_clean=batched)
        later = [c for c in im.calls if c[0] == 'clean_cycles' or (c[0] == 'clean_cycle' and c[1] != 0.0)]
        assert (not later) == stop, (metric, noise)
        assert out['peaks'] == [metric] and type(out['peaks'][0]) is np.float32
        assert out['noise'] == noise and type(out['noise']) is np.float32
        if stop:
            assert out['minor'] == 0
            continue
        assert len(im.thresholds) == (1 if batched else 3)      # (2 cycles find a peak, the third none)
        for passed in im.thresholds:
            assert F(passed).tobytes() == threshold.tobytes(), (metric, noise, passed, threshold)


@pytest.mark.parametrize('major_gain', [0.85, 0.999, 0.3])
@pytest.mark.parametrize('mode,P', HOST_MODES)
def test_host_threshold_in_one_call(mode, P, major_gain):
    """The one call: the device is handed the noise threshold as the double product of the
    float32 noise estimate and the scale, and 1 - major gain as the double it is."""
    from katsdpimager_amd import clean, frontend, weight
    inputs, want = _host_inputs(mode, P, major_gain)
    image_p, grid_p, clean_p = _host_params(mode, P, major_gain)
    scale = clean.noise_threshold_scale(mode, SIGMA, P)
    for (metric, noise), (stop, threshold) in zip(inputs, want):
        im = _Float32ShortCutRecorder(P, metric, noise)
        out = frontend.process_channel(_HostReader([1]), 0, im, image_p, grid_p, clean_p,
                                       weight.WeightType.NATURAL, 4, 1, True)
        assert len(im.handed) == 1
        noise_threshold, left = im.handed[0]
        assert float(noise_threshold) == float(noise) * scale, (noise, noise_threshold)
        assert isinstance(left, float) and left == 1.0 - major_gain
        names = [c[0] for c in im.calls]
        assert 'clean_cycle' not in names and 'clean_cycles' not in names
        # what the driver reports follows from the same comparison as the device's: the recorder
        # says 1 + 2 cycles done, the cycle that found nothing is counted where the loop went on
        assert out['peaks'] == [float(metric)]
        assert out['minor'] == (0 if stop else 3), (metric, noise)


# ---------------------------------------------------------------------------------------------
# last-ulp ladders on the device

G = 256
BORDER = 0.02               # 5 pixels: tile (ty, tx) starts at (5 + 32 ty, 5 + 32 tx)
CYCLES = 8
FIRST = (47, 49)            # tile (1, 1)
CORNERS = ((101, 133), (132, 164))      # opposite corners of tile (3, 4), 43.8 pixels apart
ALONE = (204, 89)           # tile (6, 2)
TWIN = (150, 30)            # tile (4, 0)
DEVICE_MODES = [(CLEAN_I, 1), (CLEAN_SUMSQ, 1), (CLEAN_SUMSQ, 2), (CLEAN_SUMSQ, 3)]


def _metric(mode, pixel):
    """The CLEAN metric of a pixel (float32 [P]) as include/kimg.h states it: |pol 0|, or the sum
    of squares in polarization order with every operation rounded to float32."""
    pixel = np.asarray(pixel, F)
    if mode == CLEAN_I:
        return np.abs(pixel[0])
    total = pixel[0] * pixel[0]
    for value in pixel[1:]:
        total = total + value * value
    assert type(total) is np.float32
    return total


def _ulps(value, n):
    """`value` (float32, not 0) moved by n float32 steps (towards +inf for n > 0)."""
    value = F(value)
    magnitude = int(np.abs(value).view(np.uint32)) + (n if value > 0 else -n)
    assert value != 0 and 0 < magnitude < 0x7f800000
    return np.copysign(np.uint32(magnitude).view(F), value)


def _rough_pixel(mode, P, metric, rs):
    """A pixel with about this metric: most of it in the first polarization, the last one small
    (its square then moves the sum in steps finer than an ulp of the sum)."""
    signs = rs.choice([-1.0, 1.0], P)
    if mode == CLEAN_I:
        return (signs * metric).astype(F)
    share = {1: [1.0], 2: [0.9, 0.1], 3: [0.8, 0.14, 0.06]}[P]
    return (signs * np.sqrt(np.array(share) * float(metric))).astype(F)


def _pixel_with_metric(mode, P, metric, rs):
    """A pixel whose float32 metric is exactly `metric`, or None: float32 neighbours of the last
    polarization are scanned (for one polarization few float32 values are a rounded square)."""
    pixel = _rough_pixel(mode, P, metric, rs)
    if mode == CLEAN_I:
        return pixel
    partial = float(_metric(mode, pixel[:-1])) if P > 1 else 0.0
    start = F(math.copysign(math.sqrt(max(float(metric) - partial, 0.0)), pixel[-1]))
    reach = 3 if P == 1 else 256
    for n in sorted(range(-reach, reach + 1), key=abs):
        pixel[-1] = _ulps(start, n)
        if _metric(mode, pixel) == metric:
            return pixel.copy()
    return None


def _image(P, pixels):
    dirty = np.zeros((P, G, G), F)
    for (y, x), pixel in pixels:
        dirty[:, y, x] = pixel
    return dirty


def _delta_psf(P):
    psf = np.zeros((P, G, G), F)
    psf[:, G // 2, G // 2] = 1.0
    return psf


def _two_steps(mode, P, dirty, stop, threshold):
    """The reference's two steps on the restated CleanHost: components, residual, model, tiles."""
    img, model = dirty.copy(), np.zeros_like(dirty)
    ref = orc.Clean(G, BORDER, 1.0, mode, img, _delta_psf(P), model)
    ref.reset()
    patch = (P, 9, 9)
    v, pos, pix = ref(patch, 0.0)
    log = [(v, ref.last_pos, np.array(pix))]
    if not stop:
        for _ in range(CYCLES - 1):
            v, pos, pix = ref(patch, F(threshold))
            if v is None:
                break
            log.append((v, ref.last_pos, np.array(pix)))
    return log, img, model, ref._tile_max, ref._tile_pos


class _Case:
    """One image and what has to come of it."""

    def __init__(self, mode, P, dirty, noise, sigma, major_gain, first_metric):
        from katsdpimager_amd import clean
        self.mode, self.P, self.dirty = mode, P, dirty
        self.noise, self.sigma, self.major_gain = F(noise), sigma, major_gain
        self.noise_threshold = float(self.noise) * clean.noise_threshold_scale(mode, sigma, P)
        self.left = 1.0 - major_gain
        self.stop, self.threshold = expected_threshold(mode, P, first_metric, noise, sigma, major_gain)
        self.want = _two_steps(mode, P, dirty, self.stop, self.threshold)
        assert self.want[0][0][0] == first_metric and self.want[0][0][1] == FIRST


def _ladder_case(mode, P, k, rs):
    """First peak, then rungs one ulp above, on and one ulp below the threshold that follows from
    it.  Even k: the major gain decides; odd k: the noise threshold does."""
    from katsdpimager_amd import clean
    sigma = SIGMA
    scale = float(clean.noise_threshold_scale(mode, sigma, P))
    major_gain = 0.85 if k % 2 else (0.85, 0.999, 0.3)[(k // 2) % 3]
    # the threshold's metric lies just above 2 x 4^n: consecutive float32 values x there have
    # squares 1.41 to 1.44 ulps apart, the only place where three float32 neighbours can all be
    # the rounded square of a float32 (what one polarization's sum of squares needs)
    flux = math.sqrt(rs.uniform(2.005, 2.08) * 4.0 ** rs.randint(-1, 2))
    if k % 2:
        ratio = rs.uniform(0.3, 0.8)
        power = flux / ratio
        noise0 = F(ratio * power / scale)
    else:
        power = flux / (1.0 - major_gain)
        noise0 = F(0.1 * (1.0 - major_gain) * power / scale)
    first0 = _rough_pixel(mode, P, clean.power_to_metric(mode, power), rs)
    for step in range(20000):
        first = first0.copy()
        # (float32 neighbours of whatever decides the threshold)
        first[-1] = _ulps(first0[-1], 0 if k % 2 else step)
        noise = _ulps(noise0, step if k % 2 else 0)
        metric = _metric(mode, first)
        stop, t = expected_threshold(mode, P, metric, noise, sigma, major_gain)
        if stop or t == float32_threshold(mode, P, metric, noise, sigma, major_gain):
            continue
        targets = [_ulps(t, 1), t, _ulps(t, -1)]
        rungs = []
        for m in targets:
            rungs.append(_pixel_with_metric(mode, P, m, rs))
            if rungs[-1] is None:
                break
        else:
            break
    else:
        raise AssertionError('no ladder found for mode {} P {} case {}'.format(mode, P, k))
    assert [_metric(mode, r) for r in rungs] == targets and targets[2] < t < targets[0] < metric
    decides = F(clean.power_to_metric(mode, float(noise) * scale)) == t
    assert decides == bool(k % 2)
    # rungs inside one tile and in different tiles
    places = [CORNERS[0], CORNERS[1], ALONE] if k % 4 < 2 else [ALONE, CORNERS[0], CORNERS[1]]
    dirty = _image(P, [(FIRST, first)] + list(zip(places, rungs)))
    case = _Case(mode, P, dirty, noise, sigma, major_gain, metric)
    # first peak, the rung above and the rung on the threshold; one ulp of threshold either way
    # is one component fewer or more
    assert [c[0] for c in case.want[0]] == [metric, targets[0], targets[1]]
    assert [c[1] for c in case.want[0]] == [FIRST, places[0], places[1]]
    assert np.count_nonzero(case.want[1]) == P
    assert len(_two_steps(mode, P, dirty, False, _ulps(t, 1))[0]) == 2
    assert len(_two_steps(mode, P, dirty, False, _ulps(t, -1))[0]) == 4
    return case


def _equality_cases(mode, P, rs):
    """power <= T with equality -- the loop stops after the first cycle -- and the neighbour
    where it goes on, by one ulp of a double (major gain 0 and 2^-53: T is the power itself, or
    the double below it, which still rounds to the first peak's own float32 metric) or by one ulp
    of the noise estimate (CLEAN_I with 4 sigma: the product is exact).  A second pixel with the
    first one's metric is taken where the loop goes on and stays where it does not."""
    first = _rough_pixel(mode, P, F(rs.uniform(1.1, 1.9)), rs)
    metric = _metric(mode, first)
    below = _pixel_with_metric(mode, P, _ulps(metric, -1), rs)
    pixels = [(FIRST, first), (TWIN, first)]
    if below is not None:
        pixels.append((ALONE, below))
    dirty = _image(P, pixels)
    cases = [_Case(mode, P, dirty, 0.01, SIGMA, 0.0, metric),
             _Case(mode, P, dirty, 0.01, SIGMA, 2.0 ** -53, metric)]
    assert cases[0].left == 1.0 and cases[0].stop and len(cases[0].want[0]) == 1
    assert cases[1].left < 1.0 and not cases[1].stop and cases[1].threshold == metric
    assert [c[1] for c in cases[1].want[0]] == [FIRST, TWIN]
    if mode == CLEAN_I:
        assert below is not None
        quarter = F(float(metric) / 4.0)
        assert float(quarter) * 4.0 == float(metric)
        cases += [_Case(mode, P, dirty, quarter, 4.0, 0.85, metric),
                  _Case(mode, P, dirty, _ulps(quarter, -1), 4.0, 0.85, metric)]
        assert cases[2].stop and len(cases[2].want[0]) == 1
        assert not cases[3].stop and cases[3].threshold == _ulps(metric, -1)
        assert [c[1] for c in cases[3].want[0]] == [FIRST, TWIN, ALONE]
    return cases


@functools.lru_cache(maxsize=None)
def _cases(mode, P):
    rs = np.random.RandomState(77 + 10 * mode + P)
    cases = [_ladder_case(mode, P, k, rs) for k in range(12)]
    if mode == CLEAN_I:
        assert {np.sign(c.dirty[0][FIRST]) for c in cases} == {-1.0, 1.0}
    elif P > 1:
        # where the noise decides, the threshold reaches the host as a NumPy float64: some of these
        # round DOWN to the float32 the rung sits on (a comparison in doubles would leave that rung;
        # with one polarization the scale is SIGMA, whose float32 lies below it, and a threshold on
        # which the two arithmetics disagree is one that rounds up)
        assert any(float(c.threshold) < float(c.noise_threshold) ** 2 for c in cases[1::2])
    return cases + _equality_cases(mode, P, rs)


@pytest.mark.parametrize('mode,P', DEVICE_MODES)
def test_ladders_are_sensitive(mode, P):
    """The set-up's own conditions (asserted where the cases are made), without a device."""
    cases = _cases(mode, P)
    assert len(cases) >= 14
    assert sum(1 for c in cases if c.stop) >= 1


_fns = {}


def _fn(mode, P, tuning, dirty, masked=False, slot=0):
    """A Clean of this tuning holding `dirty` (one is made per tuning and `slot`, and used again)."""
    from test_clean_mask import device_mask
    from test_clean_multi_gpu import _clean
    key = (mode, P, tuple(sorted((tuning or {}).items())), slot)
    if key not in _fns:
        _fns[key] = _clean(G, P, mode, BORDER, 1.0, dirty, _delta_psf(P), tuning)
    fn, q = _fns[key]
    fn.buffer('dirty').set(q, dirty)
    fn.buffer('model').zero(q)
    fn.bind(mask=device_mask(q, np.ones((G, G), np.uint8)) if masked else None)
    fn.reset()
    return fn, q


def _first_then(fn, case, rest):
    """The first cycle by Clean.__call__, then -- if the threshold says so -- `rest`."""
    got = [fn((case.P, 9, 9), 0.0)]
    assert got[0][0] is not None
    if not case.stop:
        got += rest(float(case.threshold))
    return got


def _per_call(fn, case):
    def rest(threshold):
        log = []
        for _ in range(CYCLES - 1):
            v, pos, pix = fn((case.P, 9, 9), threshold)
            if v is None:
                break
            log.append((v, pos, pix))
        return log
    return _first_then(fn, case, rest)


@gpu
@pytest.mark.parametrize('tuning', [{'form': 'multi'}, {'form': 'auto', 'repeats_always': True},
                                    {'form': 'multi', 'components': 1}], ids=str)
@pytest.mark.parametrize('mode,P', DEVICE_MODES)
def test_ladder_in_one_call(mode, P, tuning):
    """kimg_clean_major_cycles works the threshold out on the device: to the last bit."""
    from test_clean_multi_gpu import _check
    for case in _cases(mode, P):
        fn, q = _fn(mode, P, tuning, case.dirty)
        assert fn.run_major_cycles((P, 9, 9), case.noise_threshold, case.left, CYCLES)
        values, positions, pixels = fn._collect_cycle_arrays()
        got = [(values[i], tuple(positions[i]), pixels[i]) for i in range(len(values))]
        _check(fn, q, got, case.want)


@gpu
@pytest.mark.parametrize('form', ['two_launch', 'one_launch', 'persistent', 'one_workgroup', 'multi',
                                  'auto'])
@pytest.mark.parametrize('mode,P', DEVICE_MODES)
def test_ladder_host_threshold_then_loop(mode, P, form):
    """Every form of the device-resident loop stops at `metric < threshold`, not at `<=`."""
    from test_clean_multi_gpu import _check
    for case in _cases(mode, P):
        fn, q = _fn(mode, P, {'form': form}, case.dirty)
        got = _first_then(fn, case, lambda t: fn.run_cycles((P, 9, 9), t, CYCLES - 1))
        _check(fn, q, got, case.want)


@gpu
@pytest.mark.parametrize('mode,P', DEVICE_MODES)
def test_ladder_per_call(mode, P):
    from test_clean_multi_gpu import _check
    for case in _cases(mode, P):
        fn, q = _fn(mode, P, None, case.dirty)
        _check(fn, q, _per_call(fn, case), case.want)


@gpu
@pytest.mark.parametrize('form', ['per_call', 'two_launch', 'one_launch'])
@pytest.mark.parametrize('mode,P', DEVICE_MODES)
def test_ladder_under_a_mask_of_ones(mode, P, form):
    """A mask that allows every pixel changes nothing, at the last ulp either."""
    from test_clean_multi_gpu import _check
    for case in _cases(mode, P):
        fn, q = _fn(mode, P, None if form == 'per_call' else {'form': form}, case.dirty, masked=True)
        assert fn.buffer('mask') is not None
        if form == 'per_call':
            got = _per_call(fn, case)
        else:
            got = _first_then(fn, case, lambda t: fn.run_cycles((P, 9, 9), t, CYCLES - 1))
        _check(fn, q, got, case.want)
        fn.bind(mask=None)


@gpu
@pytest.mark.parametrize('mode,P', DEVICE_MODES)
def test_ladder_in_a_batch(mode, P):
    """Two channels with different first peaks and their own thresholds in one batch: each is its
    solo run."""
    from katsdpimager_amd import clean
    from test_clean_multi_gpu import _check
    cases = [c for c in _cases(mode, P) if not c.stop]
    for a, b in zip(cases, cases[1:]):
        assert a.threshold != b.threshold or a.want[0][0][0] != b.want[0][0][0]
        fa, q = _fn(mode, P, {'form': 'auto'}, a.dirty)
        fb, q = _fn(mode, P, {'form': 'auto'}, b.dirty, slot=1)
        assert fa is not fb
        patch = (P, 9, 9)
        got = [[f(patch, 0.0)] for f in (fa, fb)]
        assert clean.batch_supported(fa, patch)
        rest = clean.run_cycles_batch([fa, fb], [patch, patch], [float(a.threshold), float(b.threshold)],
                                      [CYCLES - 1, CYCLES - 1])
        _check(fa, q, got[0] + rest[0], a.want)
        _check(fb, q, got[1] + rest[1], b.want)


# ---------------------------------------------------------------------------------------------
# the driver's routes on one device image

class _CleanImager(_Recorder):
    """_Recorder whose CLEAN calls go to a real clean.Clean, as Imaging's do; the noise estimate is
    a fixed float32 and every make_dirty finds the same image."""

    def __init__(self, fn, q, case, one_call):
        super().__init__(num_pols=case.P)
        self._fn, self._q, self._case = fn, q, case
        if one_call:
            self.one_call_major_cycles = True
        self.components = []

    def psf_patch(self):
        return (self._case.P, 9, 9)

    def clear_model(self):
        self._fn.buffer('model').zero(self._q)

    def clear_dirty(self):
        self._fn.buffer('dirty').set(self._q, self._case.dirty)

    def noise_est(self):
        return self._case.noise

    def clean_reset(self):
        self._fn.reset()

    def clean_cycle(self, psf_patch, threshold=0.0):
        value, pos, pixel = self._fn(psf_patch, threshold)
        if pos is not None:
            self.components.append((value, pos, pixel))
        return value

    def clean_cycles(self, psf_patch, threshold, max_cycles, batcher=None):
        got = self._fn.run_cycles(psf_patch, threshold, max_cycles)
        self.components += got
        return [c[0] for c in got]

    def clean_major_cycles(self, psf_patch, noise_threshold, left_for_next, max_cycles, batcher=None):
        got = self._fn.run_major_cycles(psf_patch, noise_threshold, left_for_next, max_cycles)
        assert got
        values, positions, pixels = self._fn._collect_cycle_arrays()
        assert got[0] == len(values) and got[1] == values[0]
        self.components += [(values[i], tuple(positions[i]), pixels[i]) for i in range(len(values))]
        return got[1], got[0]


@gpu
@pytest.mark.parametrize('mode,P', DEVICE_MODES)
def test_driver_routes_agree(mode, P):
    """frontend.process_channel with one major cycle, by the one call, by the two steps with the
    device-resident loop and by the two steps with a host round trip per cycle: the same peaks,
    cycle count, components and model, and all of it the restated CleanHost's."""
    from katsdpimager_amd import frontend, weight
    from test_clean_multi_gpu import _check
    routes = [dict(one_call=True, batched=True), dict(one_call=False, batched=True),
              dict(one_call=False, batched=False)]
    for case in _cases(mode, P):
        image_p, grid_p, clean_p = _host_params(mode, P, case.major_gain, minor=CYCLES)
        clean_p.threshold = case.sigma
        later = len(case.want[0]) - 1
        # (the reference counts the cycle that found the peak below threshold too)
        minor = 0 if case.stop else later + (1 if later < CYCLES - 1 else 0)
        for route in routes:
            fn, q = _fn(mode, P, {'form': 'auto'}, case.dirty)
            im = _CleanImager(fn, q, case, route['one_call'])
            out = frontend.process_channel(_HostReader([1]), 0, im, image_p, grid_p, clean_p,
                                           weight.WeightType.NATURAL, 4, 1, True,
                                           batched_clean=route['batched'])
            assert [float(v) for v in out['peaks']] == [float(case.want[0][0][0])], route
            assert out['minor'] == minor and out['major'] == 1, (route, out['minor'], minor)
            _check(fn, q, im.components, case.want)
