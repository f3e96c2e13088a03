"""Shared by test_source_maps_host.py and test_source_maps_gpu.py: a restatement of the "Per-source
moment maps" contract of include/kimg.h that is independent of the twin -- one source at a time, every
voxel but its own blanked in a host copy of the cube, cube.moments_host over its channel range, the box
cut out -- the rows tables of the tests, and the C ABI's rejections."""
import ctypes

import numpy as np

EINVAL = -10001
EUNSUPPORTED = -10002
EWORKSPACE = -10003
KEYS = (0, 1, 2, 8, 9, 'count')
CHANNEL_WIDTH = 2.5


def coordinates(C, seed=0):
    """Descending and unevenly spaced, as velocities of ascending frequencies are."""
    rng = np.random.default_rng(1000 + seed)
    return 1500.0 - np.cumsum(rng.uniform(3.0, 5.0, C))


def restate(labels, cube, filled, rows, total, x, channel_width=CHANNEL_WIDTH):
    """{key: table of `total` entries}: per source the existing moments twin on the source's own cube."""
    from katsdpimager_amd import cube as cube_module
    C = labels.shape[0]
    out = {key: np.full(total, 0 if key == 'count' else np.nan, np.int32 if key == 'count' else np.float32)
           for key in KEYS}
    cut = np.full(C, -np.inf, np.float32)
    for s, row in enumerate(rows, 1):
        c0, c1, p, y0, x0, h, w = (int(row[name]) for name in ('c0', 'c1', 'pol', 'y0', 'x0', 'h', 'w'))
        own = np.where(labels == s, cube, np.float32(np.nan))
        params = cube_module.MomentParameters(moments=(0, 1, 2, 8, 9), axis='frequency', channels=(c0, c1 + 1))
        maps = cube_module.moments_host(own, x, cut, filled, params, channel_width)
        at = int(row['offset'])
        for key in KEYS:
            box = maps[key][p, y0:y0 + h, x0:x0 + w].reshape(-1)
            stop = min(at + h * w, total)
            if stop > at:
                out[key][at:stop] = box[:stop - at]
    return out


def measured_rows(labels, cube, filled, x, channel_width=CHANNEL_WIDTH):
    """(rows, total) of a label cube: boxes and ranges as link.measure_host finds them."""
    from katsdpimager_amd import link, source_maps
    N = int(labels.max()) if labels.size else 0
    table = link.measure_host(labels, cube, filled, N)
    catalogue = link.catalogue_host(table, labels.shape)
    return source_maps.source_rows(*(catalogue[name] for name in ('polarization', 'y0', 'y1', 'x0', 'x1', 'c0', 'c1')),
                                   x, channel_width)


def linked(mask, filled, reach, cube, x):
    """(labels, rows, total) of a mask."""
    from katsdpimager_amd import link
    labels, _ = link.link_host(mask, filled, *reach)
    return (labels,) + measured_rows(labels, cube, filled, x)


def whole_plane_rows(shape, N, x):
    """Rows for hand-made labels: source s lives in polarization (s - 1) % P, its box the whole plane
    and its range the whole band."""
    from katsdpimager_amd import source_maps
    C, P, H, W = shape
    n = np.arange(N)
    zero = np.zeros(N, np.int64)
    return source_maps.source_rows(n % P, zero, zero + H - 1, zero, zero + W - 1, zero, zero + C - 1, x,
                                   CHANNEL_WIDTH)


def random_labels(shape, N, seed):
    """Per voxel a label from 0 .. N, but only labels of the voxel's own polarization (or 0): every
    pixel leaves and resumes several sources along the channel axis."""
    C, P, H, W = shape
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, N + 1, size=shape).astype(np.int32)
    p = np.arange(P).reshape(1, P, 1, 1)
    return np.where((labels > 0) & ((labels - 1) % P != p), 0, labels).astype(np.int32)


def assert_tables(got, want, where):
    from link_cases import assert_same_bits
    assert set(got) == set(want), (where, set(got), set(want))
    for key in want:
        assert_same_bits(got[key], want[key], (where, key))


def host_ptr(array):
    return array.ctypes.data_as(ctypes.c_void_p)


def abi_rejections(lib, labels, cube, x, rows, state, out, filled, stream=None):
    """[(name, got, want)] for the argument checks of the two entries.  labels, cube: device pointers
    (c_void_p) of dense [4][16] arrays (a plane of (1, 4, 4)); x: device, 4 doubles; rows: device, two
    rows whose boxes hold 4 entries each; state: device, 8 * 36 bytes; out: device, room for six tables of
    64 bytes; filled: a host pointer of 4097 bytes."""
    P = ctypes.c_void_p
    plus = lambda p, n: P(p.value + n)
    tables = [plus(out, 64 * k) for k in range(6)]
    calls = []

    def maps(want, labels=labels, label_pitch=16, cube=cube, pitch=16, C=4, shape=(1, 4, 4), filled=filled, x=x,
             N=2, rows=rows, total=8, state=state, state_bytes=8 * 36):
        calls.append(('maps', lib.kimg_cube_source_maps(labels, label_pitch, cube, pitch, C, *shape, filled, x, N,
                                                        rows, total, state, state_bytes, stream), want))

    maps(0)
    maps(0, N=0)
    maps(0, total=0)
    maps(0, total=0, state_bytes=0)
    for name in ('labels', 'cube', 'filled', 'x', 'rows', 'state'):
        maps(EINVAL, **{name: None})
    maps(EINVAL, labels=plus(labels, 2))
    maps(EINVAL, cube=plus(cube, 1))
    maps(EINVAL, x=plus(x, 4))
    maps(EINVAL, rows=plus(rows, 4))
    maps(EINVAL, state=plus(state, 4))
    maps(EINVAL, C=0)
    maps(EINVAL, shape=(0, 4, 4))
    maps(EINVAL, shape=(1, 0, 4))
    maps(EINVAL, shape=(1, 4, 0))
    maps(EINVAL, N=-1)
    maps(EINVAL, total=-1)
    maps(EINVAL, label_pitch=15)
    maps(EINVAL, pitch=15)
    maps(EUNSUPPORTED, C=4097)
    maps(EUNSUPPORTED, C=2, shape=(1, 2 ** 15, 2 ** 15), label_pitch=2 ** 30, pitch=2 ** 30)
    maps(EUNSUPPORTED, total=2 ** 31 - 1, state_bytes=2 ** 40)
    maps(EWORKSPACE, state_bytes=8 * 36 - 1)

    def finish(want, N=2, rows=rows, total=8, state=state, state_bytes=8 * 36, x=x, C=4, outputs=63,
               tables=tables):
        calls.append(('finish', lib.kimg_source_maps_finish(N, rows, total, state, state_bytes, x, C, outputs,
                                                            *tables, stream), want))

    finish(0)
    finish(0, N=0)
    finish(0, total=0)
    finish(0, outputs=1, tables=tables[:1] + [None] * 5)
    for name in ('rows', 'state', 'x'):
        finish(EINVAL, **{name: None})
    finish(EINVAL, rows=plus(rows, 4))
    finish(EINVAL, state=plus(state, 4))
    finish(EINVAL, x=plus(x, 4))
    finish(EINVAL, N=-1)
    finish(EINVAL, total=-1)
    finish(EINVAL, C=0)
    finish(EINVAL, outputs=0)
    finish(EINVAL, outputs=64)
    finish(EINVAL, outputs=63 | 128)
    finish(EINVAL, tables=tables[:2] + [None] + tables[3:])
    finish(EINVAL, tables=tables[:5] + [plus(tables[5], 2)])
    finish(EUNSUPPORTED, C=4097)
    finish(EUNSUPPORTED, total=2 ** 31 - 1, state_bytes=2 ** 40)
    finish(EWORKSPACE, state_bytes=8 * 36 - 1)

    calls.append(('bytes', lib.kimg_cube_source_maps_workspace_bytes(8), 8 * 36))
    calls.append(('bytes', lib.kimg_cube_source_maps_workspace_bytes(0), 0))
    calls.append(('bytes', lib.kimg_cube_source_maps_workspace_bytes(-1), 0))
    calls.append(('bytes', lib.kimg_cube_source_maps_workspace_bytes(2 ** 31 - 1), 0))
    return calls
