"""The planes and blocks of test_rfiflag_host.py and test_rfiflag_gpu.py: hand-made planes whose
answer is known by construction, the noisy blocks the device is run on, and the contract of
``kimg_rfi_flag`` once more as plain loops over single samples (:func:`by_loops`), which shares no
line with the vectorised twin."""
import numpy as np

#: one row, partial / whole / whole + 1 waves (at one polarization), several workgroups
ROWS = [1, 63, 64, 65, 1000]
POLS = [1, 2, 3, 4]
TIME_BINS = [1, 3, 64]
DIRECTIONS = ['time', 'freq', 'both']
LEVEL_ITERATIONS = [0, 4, 2]


def channels(max_window):
    """The channel counts at which a window of max_window samples does not fit, just fits, fits
    twice, and a band longer than any window."""
    return sorted({1, 2, max(max_window - 1, 1), max_window, max_window + 1, 65})


def ones(C, T, P=1, groups=1):
    """(vis, weights, ids): `groups` baselines of T rows, every z exactly 1."""
    N = T * groups
    return (np.ones((C, N, P), np.complex64), np.ones((C, N, P), np.float32),
            np.repeat(np.arange(groups, dtype=np.int32), T))


def put(vis, weights, c, r, p, z):
    """Sample (c, r, p) gets z exactly: a weight of z (a small integer) under a visibility of 1."""
    vis[c, r, p] = 1.0
    weights[c, r, p] = z


def baselines(rng, N):
    """Ids of runs of 1 to 150 rows (statwt_cases.baselines)."""
    ids = []
    while len(ids) < N:
        ident = int(rng.integers(0, 6))
        if ids and ident == ids[-1]:
            ident += 6
        ids += [ident] * int(rng.integers(1, 151))
    return np.array(ids[:N], np.int32)


def inputs(C, N, P, seed, protect=True):
    """(vis, weights, ids, mask): noise of sigma 1 under weights U(0.5, 2) with 20 % zeros, some
    negative weights, NaN and Inf; channels protected in the middle of bands of 5 and more, one of
    them bright and constant; and, embedded wherever the block has room: single spikes, a run of
    four raised samples along frequency and one along time, a row and a channel hit in most of
    their samples, and rows without any weight (a skipped group where they cover one)."""
    rng = np.random.default_rng(seed)
    ids = baselines(rng, N)
    vis = (rng.normal(size=(C, N, P)) + 1j * rng.normal(size=(C, N, P))).astype(np.complex64)
    weights = rng.uniform(0.5, 2.0, (C, N, P)).astype(np.float32)
    mask = np.ones(C, np.uint8)
    if protect and C >= 5:
        mask[C // 2:C // 2 + 2] = 0
        vis[C // 2] = 40.0 - 30.0j
    for _ in range(max(1, C * N * P // 200)):                   # spikes
        vis[rng.integers(C), rng.integers(N), rng.integers(P)] *= np.float32(rng.uniform(4.0, 30.0))
    if C >= 6:                                                  # a run along frequency
        r, c = int(rng.integers(N)), int(rng.integers(C - 3))
        vis[c:c + 4, r, 0] = 2.5 + 0.5j
    if N >= 8:                                                  # ... and along time
        r, c = int(rng.integers(N - 3)), int(rng.integers(C))
        vis[c, r:r + 4, P - 1] = -2.5 + 0.5j
    for r in rng.integers(N, size=max(1, N // 40)):             # broadband bursts
        vis[:, r, rng.integers(P)] *= np.float32(6.0)
    if N >= 16:                                                 # a channel bad for a long time
        r = int(rng.integers(N - 15))
        vis[rng.integers(C), r:r + 16, 0] *= np.float32(8.0)
    weights[rng.random((C, N, P)) < 0.2] = 0.0
    for _ in range(max(1, C * N * P // 300)):
        where = (rng.integers(C), rng.integers(N), rng.integers(P))
        kind = rng.integers(4)
        if kind == 0:
            weights[where] = -1.5
        elif kind == 1:
            weights[where] = np.inf
        elif kind == 2:
            vis[where] = complex(np.nan, 2.0)
        else:
            vis[where] = complex(-1.0, np.inf)
    if N >= 3:                                                  # rows without weight
        r = int(rng.integers(N - 2))
        weights[:, r:r + 3, P - 1] = 0.0
    return vis, weights, ids, mask


#: the hot run of band_inputs: 32 channels that straddle the seam between words 1 and 2 of the mask
HOT = (48, 80)
BRIGHT = 32


def band_inputs(C, N, P, seed, mask):
    """(vis, weights, ids, mask) for a band of more than 80 channels: the noise and the embedded
    features of :func:`inputs` with the protected channels of ``mask`` (0 = protected; band_cases.py)
    instead of the middle of the band; channel 32, the first of word 1, protected as well, bright and
    constant; and in one row of polarization 0 a run of 32 usable samples, channels 48 to 79, at
    z = 12, about five times the noise's level (1.25 x 2): the windows that hold them lie across the
    seam between words 1 and 2 of the mask at channel 64, the one window of 32 that holds them all
    among them.  The row is the middle one of the longest run of one baseline; it and the two rows on
    either side of it (its group at time_bin 3, whichever that is) are plain noise without zero
    weights in polarization 0, so that no burst of :func:`inputs` lifts the group's level over the run."""
    vis, weights, ids, _ = inputs(C, N, P, seed, protect=False)
    mask = np.array(mask, np.uint8)
    mask[BRIGHT] = 0
    vis[BRIGHT] = 40.0 - 30.0j
    row = hot_row(ids)
    rng = np.random.default_rng(seed + 1)
    near = slice(max(row - 2, 0), min(row + 3, N))
    shape = vis[:, near, 0].shape
    vis[:, near, 0] = (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(np.complex64)
    weights[:, near, 0] = rng.uniform(0.5, 2.0, shape).astype(np.float32)
    vis[BRIGHT] = 40.0 - 30.0j
    vis[HOT[0]:HOT[1], row, 0] = np.complex64(np.sqrt(12.0))
    weights[HOT[0]:HOT[1], row, 0] = 1.0
    return vis, weights, ids, mask


def hot_row(ids):
    """The row that holds the hot run of band_inputs: the middle of the longest run of one id."""
    edges = np.flatnonzero(np.diff(ids)) + 1
    starts = np.concatenate(([0], edges))
    stops = np.concatenate((edges, [len(ids)]))
    g = int(np.argmax(stops - starts))
    return int(starts[g] + stops[g]) // 2


def by_loops(vis, weights, ids, params):
    """``kimg_rfi_flag`` as include/kimg.h words it, one sample at a time in Python floats (IEEE
    float64, like the contract): (weights, flags, level, counts).  For small blocks."""
    from katsdpimager_amd import statwt
    C, N, P = vis.shape
    mask = params.mask(C)
    offsets = statwt.group_offsets(ids, params.time_bin)
    G = len(offsets) - 1
    factors = [float(f) for f in params.factors()]
    flags = np.zeros((C, N, P), bool)
    level = np.full((G, P), np.nan)
    usable = np.zeros((C, N, P), bool)
    z = np.zeros((C, N, P))
    for c in range(C):
        for r in range(N):
            for p in range(P):
                w, v = weights[c, r, p], vis[c, r, p]
                if w > 0 and np.isfinite(w) and np.isfinite(v.real) and np.isfinite(v.imag):
                    usable[c, r, p] = True
                    re, im = float(v.real), float(v.imag)
                    t = re * re
                    t = t + im * im
                    z[c, r, p] = float(w) * t
    skipped = 0
    for g in range(G):
        rows = range(offsets[g], offsets[g + 1])
        for p in range(P):
            def search(c, r):
                return mask[c] and usable[c, r, p]

            # the level
            limit, L, alive = np.inf, None, True
            for _ in range(params.level_iterations + 1):
                Z, M = 0.0, 0
                for r in rows:
                    zrow = 0.0
                    for c in range(C):
                        if search(c, r) and z[c, r, p] <= limit:
                            zrow += z[c, r, p]
                            M += 1
                    Z += zrow
                L = Z / M if M else np.nan
                if not (M > 0 and np.isfinite(L) and L > 0):
                    alive = False
                    break
                limit = params.level_clip * L
            if not alive:
                skipped += 1
                continue
            level[g, p] = L
            for k, factor in enumerate(factors):
                m = 1 << k
                chi = factor * L
                entered = flags[:, :, p].copy()
                windows = []
                if params.directions in ('freq', 'both'):
                    windows += [[(c, r) for c in range(s, s + m)] for r in rows for s in range(C - m + 1)]
                if params.directions in ('time', 'both'):
                    windows += [[(c, r) for r in range(s, s + m)] for c in range(C) if mask[c]
                                for s in range(rows[0], rows[-1] + 2 - m)]
                for window in windows:
                    total, own = 0.0, 0
                    for c, r in window:
                        if search(c, r) and not entered[c, r]:
                            total = total + (z[c, r, p] - L)
                            own += 1
                        else:
                            total = total + chi
                    if own and total > float(m) * chi:
                        for c, r in window:
                            if search(c, r):
                                flags[c, r, p] = True
    alive = ~np.isnan(level)
    if params.extend_freq is not None:
        for g in range(G):
            for p in range(P):
                for r in range(offsets[g], offsets[g + 1]):
                    have = sum(1 for c in range(C) if mask[c] and usable[c, r, p])
                    hit = sum(1 for c in range(C) if mask[c] and usable[c, r, p] and flags[c, r, p])
                    if alive[g, p] and float(hit) > params.extend_freq * float(have):
                        flags[:, r, p] |= usable[:, r, p]
    if params.extend_time is not None:
        for g in range(G):
            rows = slice(offsets[g], offsets[g + 1])
            for p in range(P):
                for c in np.flatnonzero(mask):
                    have = int(usable[c, rows, p].sum())
                    hit = int((usable[c, rows, p] & flags[c, rows, p]).sum())
                    if float(hit) > params.extend_time * float(have):
                        flags[c, rows, p] |= usable[c, rows, p]
    if params.extend_pols:
        group = statwt._row_groups(offsets)
        anywhere = flags.any(axis=2)
        for p in range(P):
            flags[:, :, p] |= anywhere & usable[:, :, p] & alive[group, p][None]
    out = weights.copy()
    out[flags] = 0.0
    flagged = int(flags.sum())
    return out, flags.astype(np.uint8), level, (int(usable.sum()) - flagged, flagged, skipped)


def assert_same(got, want):
    """Two results (weights, flags, level, counts) agree to the bit."""
    assert np.array_equal(got[1], want[1]), 'flags'
    assert got[1].dtype == np.uint8 and got[0].dtype == np.float32 and got[2].dtype == np.float64
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), 'weights'
    nan = np.isnan(want[2])
    assert got[2].shape == want[2].shape and np.array_equal(np.isnan(got[2]), nan), 'skipped'
    assert np.array_equal(got[2][~nan].view(np.uint64), want[2][~nan].view(np.uint64)), 'level'
    assert tuple(got[3]) == tuple(want[3]), (got[3], want[3])
