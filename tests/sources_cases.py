"""Shared by test_sources_host.py and test_sources_gpu.py: a plain-Python restatement of the "Source
spectra and line parameters" contracts of include/kimg.h (a loop per source, math.fsum for the sums),
a SpectralCube without a device behind it, and the C ABI's rejections."""
import ctypes
import math

import numpy as np

EINVAL = -10001
EUNSUPPORTED = -10002
LINE_DOUBLES = ('flux', 'flux_err', 'peak', 'centroid', 'w50', 'w20', 'w50_lo', 'w50_hi', 'w20_lo', 'w20_hi')


def restate_spectra(labels, cube, filled, c0, offsets):
    """Source by source, channel by channel: (fsum, voxels, finite, sum |term|) lists of offsets[-1]
    entries."""
    total = int(offsets[-1])
    sums, voxels, finite, magnitude = [0.0] * total, [0] * total, [0] * total, [0.0] * total
    C = labels.shape[0]
    for s in range(1, len(c0) + 1):
        for at in range(int(offsets[s - 1]), int(offsets[s])):
            c = int(c0[s - 1]) + at - int(offsets[s - 1])
            if not 0 <= c < C or not filled[c] or not 0 <= at < total:
                continue
            values = cube[c][labels[c] == s]
            good = [float(v) for v in values if math.isfinite(v)]
            voxels[at] += len(values)
            finite[at] += len(good)
            sums[at] = math.fsum(good)
            magnitude[at] = math.fsum(abs(v) for v in good)
    return sums, voxels, finite, magnitude


def assert_spectra(got, labels, cube, filled, c0, offsets, exact, where, restated=None):
    """(sum, voxels, finite) against the restatement (made here unless given): counts equal; sums equal
    (`exact`) or within finite * 2^-53 * sum |term| of the fsum."""
    if restated is None:
        restated = restate_spectra(labels, cube, filled, c0, offsets)
    sums, voxels, finite, magnitude = restated
    assert list(got[1]) == voxels, (where, 'voxels')
    assert list(got[2]) == finite, (where, 'finite')
    for at in range(len(sums)):
        if exact:
            assert float(got[0][at]) == sums[at], (where, at, got[0][at], sums[at])
        else:
            bound = finite[at] * 2.0 ** -53 * magnitude[at]
            assert abs(float(got[0][at]) - sums[at]) <= bound, (where, at, got[0][at], sums[at], bound)


def host_cube(frequencies, filled, noise=None, beams=None, common_beam=None, channel_width=None):
    """A cube.SpectralCube with its host tables and no device array: what line_tables reads."""
    from katsdpimager_amd import cube
    the_cube = object.__new__(cube.SpectralCube)
    C = len(frequencies)
    the_cube.frequencies = np.array(frequencies, np.float64)
    the_cube.channel_width = channel_width
    the_cube.shape = (C, 1, 1, 1)
    the_cube.filled = np.asarray(filled, np.uint8)
    the_cube.noise = np.full(C, np.nan, np.float32) if noise is None else np.asarray(noise, np.float32)
    the_cube.beams = [None] * C if beams is None else list(beams)
    the_cube.common_beam = common_beam
    return the_cube


def plant_blanks(cube, seed):
    """NaN, +Inf and -Inf in a few voxels, in place."""
    rng = np.random.default_rng(seed)
    flat = cube.reshape(-1)
    for value, share in ((np.nan, 0.04), (np.inf, 0.01), (-np.inf, 0.01)):
        flat[rng.random(flat.size) < share] = value
    return cube


def host_ptr(array):
    return array.ctypes.data_as(ctypes.c_void_p)


def abi_rejections(lib, table_type, labels, cube, layout, tables, filled, channel, stream=None):
    """[(name, got, want)] for the argument checks of the two entries.  labels, cube: device pointers
    (c_void_p) of dense [4][16] arrays; layout: a device pointer of int32 [c0 (2)][offsets (3)] for two
    sources of 2 channels each; tables: a device pointer with room for 16 arrays of 64 bytes; filled: a
    host pointer of 4097 bytes; channel: a host pointer of 4097 doubles."""
    P = ctypes.c_void_p
    plus = lambda p, n: P(p.value + n)
    c0, offsets = layout, plus(layout, 8)
    sums, voxels, finite = tables, plus(tables, 64), plus(tables, 128)
    space = plus(tables, 192)           # 16 doubles = 4 tables of 4 channels, 128 bytes
    fields = [name for name, _ in table_type._fields_]
    good = table_type(**{name: tables.value + 320 + 64 * k for k, name in enumerate(fields)})
    null_field = table_type(**{name: (0 if name == 'peak' else tables.value + 320 + 64 * k)
                               for k, name in enumerate(fields)})
    odd_field = table_type(**{name: tables.value + 320 + 64 * k + (4 if name == 'w20' else 0)
                              for k, name in enumerate(fields)})
    ref = ctypes.byref
    calls = []

    def spectra(want, labels=labels, label_pitch=16, cube=cube, pitch=16, C=4, M=16, filled=filled, N=2,
                c0=c0, offsets=offsets, total=4, sums=sums, voxels=voxels, finite=finite):
        calls.append(('spectra', lib.kimg_cube_source_spectra(labels, label_pitch, cube, pitch, C, M, filled, N,
                                                              c0, offsets, total, sums, voxels, finite, stream),
                      want))

    spectra(0)
    spectra(0, N=0)
    spectra(0, M=0)
    spectra(0, total=0)
    for name in ('labels', 'cube', 'filled', 'c0', 'offsets', 'sums', 'voxels', 'finite'):
        spectra(EINVAL, **{name: None})
    spectra(EINVAL, labels=plus(labels, 2))
    spectra(EINVAL, cube=plus(cube, 1))
    spectra(EINVAL, offsets=plus(offsets, 2))
    spectra(EINVAL, sums=plus(sums, 4))
    spectra(EINVAL, finite=plus(finite, 2))
    spectra(EINVAL, N=-1)
    spectra(EINVAL, total=-1)
    spectra(EINVAL, label_pitch=15)
    spectra(EINVAL, pitch=15)
    spectra(EINVAL, C=0)
    spectra(EINVAL, M=-1)
    spectra(EUNSUPPORTED, C=4097)
    spectra(EUNSUPPORTED, C=2, M=2 ** 30, label_pitch=2 ** 30, pitch=2 ** 30)
    spectra(EUNSUPPORTED, total=2 ** 31 - 1)

    def lines(want, N=2, c0=c0, offsets=offsets, total=4, sums=sums, finite=finite, C=4, unit=channel,
              width=channel, coord=channel, variance=channel, space=space, table=ref(good)):
        calls.append(('lines', lib.kimg_source_lines(N, c0, offsets, total, sums, finite, C, unit, width, coord,
                                                     variance, space, table, stream), want))

    lines(0)
    lines(0, N=0)
    for name in ('c0', 'offsets', 'sums', 'finite', 'unit', 'width', 'coord', 'variance', 'space', 'table'):
        lines(EINVAL, **{name: None})
    lines(EINVAL, c0=plus(c0, 2))
    lines(EINVAL, sums=plus(sums, 4))
    lines(EINVAL, space=plus(space, 4))
    lines(EINVAL, table=ref(null_field))
    lines(EINVAL, table=ref(odd_field))
    lines(EINVAL, N=-1)
    lines(EINVAL, total=-1)
    lines(EINVAL, C=0)
    lines(EUNSUPPORTED, C=4097)
    lines(EUNSUPPORTED, total=2 ** 31 - 1)
    return calls
