"""Shared by test_imcontsub_host.py and test_imcontsub_gpu.py: the cubes both suites run, the
conditioning they are held to, the bound of the comparisons and the ABI's argument errors.

The bound, per value: |got - t| <= 2^-24 |t| + 1e-9 S, t the twin's value BEFORE its one rounding to
float32 and S the element's largest finite |I|.  It is the one tests/test_uvcontsub_gpu.py states and
derives: the first term is the one rounding the contract allows, the second covers float64 arithmetic
in another order, about K^2 cond(A) 2^-53 S = 2e-12 S at cond(A) <= 1e3, which every cube here is
asserted to keep (:func:`worst_cond`)."""
import ctypes

import numpy as np

EINVAL, EUNSUPPORTED = -10001, -10002
CHANNELS = (1, 2, 3, 8, 9, 33, 65)
#: the elements of the plane that make_cube shapes by hand, where the plane has that many
HAND_MADE = 8


def orders(C):
    """The orders a band of C channels can be fitted with."""
    return [order for order in range(4) if order + 1 <= C]


def selection(C, order):
    """(fit_mask, filled) of a band of C channels: a block of line channels in the middle where the
    band has room beside the order + 1 channels the fit needs (a quarter of a band of 8 or more), and,
    from 8 channels, one line-free and one line channel that are not filled."""
    K = order + 1
    lines = max(min(C // 4 if C >= 8 else 1, C - K), 0)
    fit = np.ones(C, np.uint8)
    first = (C - lines) // 2
    fit[first:first + lines] = 0
    filled = np.ones(C, np.uint8)
    if C >= 8:
        filled[first + lines // 2] = 0                      # a line channel
        filled[np.flatnonzero(fit)[2]] = 0                  # a line-free channel
    return fit, filled


def make_cube(C, plane, order, seed, weighting='none'):
    """``(cube, filled, fit_mask, frequencies, noise)``: per element a smooth polynomial of degree 3
    across the band plus noise, plus a line in the line channels; uneven ascending frequencies; noises
    U(0.5, 2).  With HAND_MADE elements or more in the plane, element

      0  has order usable samples in the fit channels (one too few: not fitted), where order >= 1,
      1  has order + 1 exactly, on well-spread channels,
      2  a NaN and an Inf in fit channels (where order + 3 channels enter the fit),
      3  a NaN in a line channel (where there is a filled one),
      4  is NaN in every channel,
      5  has -Inf in a line channel (where there is a filled one);

    the samples that are knocked out of 0 and 1 are NaN, Inf and -Inf in turn."""
    rng = np.random.default_rng(seed)
    K = order + 1
    fit, filled = selection(C, order)
    shape = (C,) + tuple(plane)
    M = int(np.prod(plane))
    x = np.linspace(-1.0, 1.0, C) if C > 1 else np.zeros(1)
    coefficients = rng.normal(0.0, 1.0, (4, M)) * np.array([3.0, 1.0, 0.5, 0.25])[:, None]
    smooth = sum(coefficients[k][None, :] * x[:, None] ** k for k in range(4))
    data = smooth + rng.normal(0.0, 0.1, (C, M))
    data[fit == 0] += rng.uniform(1.0, 4.0, M)[None, :]
    flat = data.astype(np.float32)
    enter = np.flatnonzero(fit & filled)
    line = np.flatnonzero((fit == 0) & (filled != 0))
    junk = (np.nan, np.inf, -np.inf)

    def keep_only(j, channels):
        for i, c in enumerate(np.setdiff1d(enter, channels)):
            flat[c, j] = junk[i % 3]
    if M >= HAND_MADE:
        spread = enter[np.round(np.linspace(0, len(enter) - 1, K)).astype(int)]
        if K >= 2:
            keep_only(0, spread[:K - 1])
        keep_only(1, spread)
        if len(enter) >= K + 2:
            flat[enter[len(enter) // 2], 2] = np.nan
            flat[enter[0], 2] = np.inf
        if len(line):
            flat[line[0], 3] = np.nan
            flat[line[-1], 5] = -np.inf
        flat[:, 4] = np.nan
    frequencies = 1.4e9 + 1.0e6 * (np.arange(C) + 0.3 * np.sin(np.arange(C)))
    noise = rng.uniform(0.5, 2.0, C).astype(np.float32)
    return flat.reshape(shape), filled, fit, frequencies, noise


def worst_cond(cube, filled, params, frequencies=None, noise=None):
    """The largest cond(A) over the elements that are fitted (1 where none is)."""
    C = cube.shape[0]
    filled, fit, w, B, _, min_samples = params.tables(C, filled, frequencies, noise)
    flat = cube.reshape(C, -1)
    usable = (fit != 0)[:, None] & np.isfinite(flat)
    wm = np.where(usable, w[:, None], 0.0)
    A = np.einsum('cm,kc,lc->mkl', wm, B, B)
    fitted = usable.sum(axis=0) >= max(params.order + 1, min_samples)
    return float(np.linalg.cond(A[fitted]).max()) if fitted.any() else 1.0


def scale(cube, filled):
    """S: the largest finite |I| of every element over the filled channels, float64 [...plane]."""
    on = (np.asarray(filled) != 0).reshape((-1,) + (1,) * (cube.ndim - 1))
    return np.where(np.isfinite(cube) & on, np.abs(cube.astype(np.float64)), 0.0).max(axis=0)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_within_bound(got, t, S, where=None):
    """``got`` (float32) against the value before rounding ``t`` (float64): NaN in the same places,
    infinities equal, everything else within 2^-24 |t| + 1e-9 S."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == t.shape, where
    S = np.broadcast_to(S, t.shape)
    nan = np.isnan(t)
    assert np.array_equal(np.isnan(got), nan), where
    inf = np.isinf(t)
    assert np.array_equal(got[inf].astype(np.float64), t[inf]), where
    ok = ~(nan | inf)
    err = np.abs(got[ok].astype(np.float64) - t[ok])
    bound = 2.0 ** -24 * np.abs(t[ok]) + 1e-9 * S[ok]
    assert (err <= bound).all(), (where, 'worst excess {:.3g}'.format(float((err - bound).max())))


def twin(cube, filled, params, frequencies=None, noise=None):
    """The twin's answers for one cube, computed once and shared by every layout that runs it:
    (unrounded line, unrounded maps, rounded line, rounded maps, S)."""
    from katsdpimager_amd import imcontsub
    t_line, t = imcontsub.imcontsub_host_double(cube, filled, params, frequencies, noise)
    r_line, r = imcontsub.imcontsub_host(cube, filled, params, frequencies, noise)
    return t_line, t, r_line, r, scale(cube, filled)


def assert_against_twin(line, maps, cube, filled, params, reference, where=None, untouched=None):
    """A result -- ``line`` float32 [C][...plane] and ``maps``, host arrays -- against ``reference``
    (:func:`twin` of the same cube): the values within the bound of the value before rounding, and
    exactly: count, the fitted set, the NaN placement, the bits of non-finite samples that are stored
    unchanged, and the channels that are not filled, which must hold ``untouched`` (default: the
    input's own bits).  Returns whether everything also has the bits of the ROUNDED twin -- which the
    device has in every case of test_imcontsub_gpu.py (the order of every float64 operation is the
    twin's, nothing is fused, and the build's float64 division and sqrt are correctly rounded), so
    that suite asserts it; the bound stays as what the contract promises a caller."""
    t_line, t, r_line, r, S = reference
    on = np.asarray(filled) != 0
    fitted = t['fitted']
    assert line.dtype == np.float32 and line.shape == cube.shape, where
    assert_within_bound(line[on], t_line[on], S[np.newaxis], where)
    kept = on.reshape((-1,) + (1,) * (cube.ndim - 1)) & fitted[np.newaxis] & ~np.isfinite(cube)
    assert np.array_equal(bits(line)[kept], bits(cube)[kept]), where
    assert np.isnan(line[on][:, ~fitted]).all(), where
    rest = cube if untouched is None else untouched
    assert np.array_equal(bits(line)[~on], bits(rest)[~on]), (where, 'an unfilled channel changed')
    same = np.array_equal(bits(line)[on][~np.isnan(r_line[on])], bits(r_line)[on][~np.isnan(r_line[on])])
    for key, got in maps.items():
        if key == 'count':
            assert got.dtype == np.int32 and np.array_equal(got, t['count']), (where, key)
            continue
        assert_within_bound(got, t[key], S, (where, key))
        assert np.array_equal(np.isnan(got), np.broadcast_to(
            ~fitted | ((t['count'] <= params.order + 1) if key == 'rms' else False), got.shape)), (where, key)
        nan = np.isnan(r[key])
        same = same and np.array_equal(bits(got)[~nan], bits(r[key])[~nan])
    return bool(same)


# ---- the longest band ------------------------------------------------------------------------------
LIMIT_CHANNELS = 4096
LIMIT_PLANE = (1, 1, 5)


def limit_case(seed=4096):
    """``(cube, filled, fit_mask, frequencies, noise)`` of LIMIT_CHANNELS x LIMIT_PLANE: the fit
    channels at both ends of the band, spread through it and in the last word of the mask (one of them
    the band's last channel); a fit channel and two line channels not filled, one of these in the last
    word; element 0 with a NaN in the band's last channel."""
    C = LIMIT_CHANNELS
    rng = np.random.default_rng(seed)
    fit = np.zeros(C, np.uint8)
    fit[[0, 1, 2, 700, 1400, 2047, 2048, 2800, 3500, C - 30, C - 2, C - 1]] = 1
    filled = np.ones(C, np.uint8)
    filled[[1400, 31, C - 9]] = 0
    x = np.linspace(-1.0, 1.0, C)
    M = int(np.prod(LIMIT_PLANE))
    coefficients = rng.normal(0.0, 1.0, (4, M))
    data = sum(coefficients[k][None, :] * x[:, None] ** k for k in range(4)) + rng.normal(0.0, 0.1, (C, M))
    data = data.astype(np.float32)
    data[C - 1, 0] = np.nan
    frequencies = 1.4e9 + 1.0e5 * np.arange(C)
    noise = rng.uniform(0.5, 2.0, C).astype(np.float32)
    return data.reshape((C,) + LIMIT_PLANE), filled, fit, frequencies, noise


# ---- the ABI's argument errors ---------------------------------------------------------------------
def abi_call(lib, **a):
    return lib.kimg_imcontsub(
        a['cube'], a['pitch'], a['line'], a['line_pitch'], a['C'], a['M'], a['filled'], a['fit'],
        a['w_host'], a['w'], a['basis'], a['order'], 1.0, 0.0, -0.5, 0.0, a['min_samples'],
        a['outputs'], a['continuum'], a['coefficients'], a['coefficient_pitch'], a['rms'], a['count'],
        a['stream'])


def abi_errors(lib, cube, line, tables, maps, C=8, M=64):
    """Every argument error of kimg_imcontsub with its code: all come before any HIP call.  ``cube``
    and ``line``: addresses of C * M floats each, 16-byte aligned, that share nothing; ``tables``: of
    5 C doubles; ``maps``: of 7 M floats.  Returns the number checked; keeps its host tables alive."""
    ones = (ctypes.c_uint8 * 4097)(*([1] * 4097))
    few = (ctypes.c_uint8 * C)(*([1, 1] + [0] * (C - 2)))
    weights = (ctypes.c_double * 4097)(*([1.0] * 4097))
    bad_weights = (ctypes.c_double * C)(*([1.0, 1.0, 0.0, -1.0, float('inf'), float('nan')] + [0.0] * (C - 6)))
    u8 = lambda table: ctypes.cast(table, ctypes.c_void_p)              # noqa: E731
    good = dict(cube=cube, pitch=M, line=line, line_pitch=M, C=C, M=M, filled=u8(ones), fit=u8(ones),
                w_host=u8(weights), w=tables, basis=tables + 8 * C, order=3, min_samples=1,
                outputs=1 | 2 | 4 | 8, continuum=maps, coefficients=maps + 4 * M, coefficient_pitch=M,
                rms=maps + 20 * M, count=maps + 24 * M, stream=None)
    assert abi_call(lib, **dict(good, M=0, pitch=0, line_pitch=0, coefficient_pitch=0)) == 0
    bad = [
        (dict(order=-1), EINVAL), (dict(order=4), EINVAL), (dict(C=0), EINVAL),
        (dict(filled=None), EINVAL), (dict(fit=None), EINVAL), (dict(w_host=None), EINVAL),
        (dict(C=4097), EUNSUPPORTED),
        # fewer than K channels enter: by the selection, by what is filled, by the weights
        (dict(fit=u8(few)), EUNSUPPORTED), (dict(filled=u8(few)), EUNSUPPORTED),
        (dict(w_host=u8(bad_weights)), EUNSUPPORTED),
        (dict(M=2 ** 31 * 256, pitch=2 ** 40, line_pitch=2 ** 40), EUNSUPPORTED),
        (dict(cube=None), EINVAL), (dict(line=None), EINVAL), (dict(w=None), EINVAL),
        (dict(basis=None), EINVAL), (dict(M=-1), EINVAL),
        (dict(min_samples=0), EINVAL), (dict(min_samples=C + 1), EINVAL),
        (dict(pitch=M - 1), EINVAL), (dict(line_pitch=M - 1), EINVAL),
        (dict(outputs=0), EINVAL), (dict(outputs=16), EINVAL), (dict(outputs=1 | 16), EINVAL),
        (dict(cube=cube + 2), EINVAL), (dict(line=line + 2), EINVAL), (dict(w=tables + 4), EINVAL),
        (dict(continuum=None), EINVAL), (dict(coefficients=None), EINVAL), (dict(rms=None), EINVAL),
        (dict(count=None), EINVAL), (dict(rms=maps + 2), EINVAL),
        (dict(coefficient_pitch=M - 1), EINVAL),
        # the line cube overlaps the cube without being it: shifted by an element, by a plane, the
        # same address under another pitch, and from the far side
        (dict(line=cube + 4, M=M - 1), EINVAL), (dict(line=cube + 4 * M), EINVAL),
        (dict(line=cube, line_pitch=M + 4, M=M - 4, pitch=M), EINVAL),
        (dict(cube=cube + 4 * M, line=cube, C=C - 1), EINVAL),
    ]
    for change, code in bad:
        got = abi_call(lib, **dict(good, **change))
        assert got == code, (change, got)
    return len(bad) + 1
