"""The blocks test_statwt_gpu.py runs the device on, made here so that test_statwt_host.py can check
without a device that every one of them holds what it was made to hold."""
import numpy as np

#: (C, fit mask): the bands of test_uvcontsub_gpu.SHAPES (their masks; the order does not matter
#: here), and one with every channel in the statistic
SHAPES = [
    (24, [1] * 9 + [0] * 6 + [1] * 9),
    (5, [1] * 5),
    (16, [1] * 6 + [0] * 4 + [1] * 6),
    (7, [1, 1, 0, 0, 0, 1, 1]),
    (1, [1]),
    (12, None),
]
#: one row, partial / whole / whole + 1 waves (at one polarization), several workgroups
ROWS = [1, 63, 64, 65, 1000]
POLS = [1, 2, 3, 4]
TIME_BINS = [1, 3, 64]
#: the outlier cut of the time_bin = 3 cases whose groups can hold 8 samples.  The noise below has
#: variance 9 per component and the weights lie in (0.5, 2), so chi2 = w * variance scatters around
#: 11, inside the range; the groups marked 'low' and 'high' are scaled by 0.01 and 100 and fall out of
#: it on either side.
CHI2_RANGE = (1.0, 60.0)


def baselines(rng, N):
    """Ids of runs of 1 to 150 rows, drawn from few values so that an id comes back later in the
    block: groups start and end inside, at and across wave and workgroup boundaries."""
    ids = []
    while len(ids) < N:
        ident = int(rng.integers(0, 6))
        if ids and ident == ids[-1]:
            ident += 6
        ids += [ident] * int(rng.integers(1, 151))
    return np.array(ids[:N], np.int32)


def parameters(C, mask, time_bin, ids):
    """(params, offsets, g, most): the parameters of a case, its groups, the largest group and the
    number of samples it can have.  min_samples = min(8, most), never below 2."""
    from katsdpimager_amd import statwt
    offsets = statwt.group_offsets(ids, time_bin)
    fit = C if mask is None else int(np.sum(mask))
    sizes = np.diff(offsets)
    g = int(np.argmax(sizes))
    most = int(sizes[g]) * fit
    params = statwt.StatWtParameters(time_bin, fit_mask=mask, min_samples=max(2, min(8, most)),
                                     chi2_range=CHI2_RANGE if time_bin == 3 and most >= 8 else None)
    return params, offsets, g, most


def inputs(C, mask, N, P, time_bin, seed):
    """(vis, weights, ids, params, marks): test_uvcontsub_gpu._inputs for this operator.  Noise of
    sigma 3, weights U(0.5, 2) with 20 % zeros, and hand-made groups, marks[name] = (g, p):
      'exact'     exactly min_samples usable samples, the others knocked out by a zero weight, a
                  negative weight, a NaN and an Inf in turn: kept.  Absent only where no group can
                  reach 2 samples (one fit channel and groups of one row).
      'empty'     every weight 0: flagged, chi2 NaN.  Absent only where the block is a single (group,
                  polarization) pair.
      'constant'  constant visibilities at weight 1, chi2 == 0: flagged.
      'low', 'high'  (under CHI2_RANGE) every fit sample usable, visibilities scaled by 0.01 and by 100:
                  flagged by either side of the range.
    The last three, and a negative weight, a NaN and an Inf in fit channels and a NaN in a line channel
    of otherwise ordinary rows, where groups and rows are left for them (any block of 1000 rows)."""
    rng = np.random.default_rng(seed)
    ids = baselines(rng, N)
    params, offsets, g_exact, most = parameters(C, mask, time_bin, ids)
    G = len(offsets) - 1
    vis = ((rng.normal(size=(C, N, P)) + 1j * rng.normal(size=(C, N, P))) * 3.0).astype(np.complex64)
    weights = rng.uniform(0.5, 2.0, (C, N, P)).astype(np.float32)
    weights[rng.random((C, N, P)) < 0.2] = 0.0
    m = params.mask(C)
    fit = np.flatnonzero(m)
    line = np.flatnonzero(m == 0)
    marks = {}
    ranged = params.chi2_range == CHI2_RANGE

    def rows_of(g):
        return np.arange(offsets[g], offsets[g + 1])

    def all_usable(g, p, value=None):
        shape = (len(fit), len(rows_of(g)), 1)
        weights[np.ix_(fit, rows_of(g), [p])] = rng.uniform(0.5, 2.0, shape) if value is None else value
    if most >= 2:
        # (under the range: weight 1, so that chi2 is near 9 whichever samples are knocked out)
        all_usable(g_exact, 0, 1.0 if ranged else None)
        samples = [(c, r) for r in rows_of(g_exact) for c in fit]
        for i, (c, r) in enumerate(samples[:most - params.min_samples]):
            if i % 4 == 0:
                weights[c, r, 0] = 0.0
            elif i % 4 == 1:
                weights[c, r, 0] = -1.5
            elif i % 4 == 2:
                vis[c, r, 0] = complex(np.nan, 2.0)
            else:
                vis[c, r, 0] = complex(-1.0, np.inf)
        marks['exact'] = (g_exact, 0)
    if G * P >= 2:
        # the last group at the last polarization, or the group before it where that pair is taken
        g_empty, p_empty = G - 1, P - 1
        if (g_empty, p_empty) == marks.get('exact'):
            g_empty = G - 2
        weights[:, rows_of(g_empty), p_empty] = 0.0
        marks['empty'] = (g_empty, p_empty)
    # groups no mark has touched (at any polarization), from the middle of the block
    free = [g for g in range(G) if g not in {pair[0] for pair in marks.values()}]
    free = free[len(free) // 3:]
    if free:
        g = free.pop(0)
        vis[:, rows_of(g), 0] = complex(1.5, -0.5)
        weights[:, rows_of(g), 0] = 1.0
        marks['constant'] = (g, 0)
    if ranged:
        for name, scale in (('low', 0.01), ('high', 100.0)):
            full = [g for g in free if len(rows_of(g)) * len(fit) >= params.min_samples]
            if full:
                g = full[0]
                free.remove(g)
                all_usable(g, 0)
                vis[:, rows_of(g), 0] *= np.float32(scale)
                marks[name] = (g, 0)
    ordinary = [r for g in free for r in rows_of(g)][:4]
    if len(ordinary) == 4:
        p = P - 1
        weights[fit[0], ordinary[0], p] = -0.75
        weights[fit[-1], ordinary[1], p] = 1.25
        vis[fit[-1], ordinary[1], p] = complex(np.nan, 1.0)
        weights[fit[len(fit) // 2], ordinary[2], p] = 0.75
        vis[fit[len(fit) // 2], ordinary[2], p] = complex(2.0, -np.inf)
        if len(line):
            weights[line[0], ordinary[3], p] = 1.5
            vis[line[0], ordinary[3], p] = complex(3.0, np.nan)
        marks['samples'] = (-1, p)
    return vis, weights, ids, params, marks


def assert_marks(marks, new_weights, chi2, counts, weights, offsets, most, N, P):
    """The twin's output says of the hand-made groups what they were made for: the case still holds
    what it was written to hold."""
    G = len(offsets) - 1
    assert ('exact' in marks) == (most >= 2)
    assert ('empty' in marks) == (G * P >= 2)
    if N == 1000:
        assert {'constant', 'samples'} <= set(marks)
    for name, (g, p) in marks.items():
        if name == 'samples':
            continue
        rows = slice(offsets[g], offsets[g + 1])
        out, before = new_weights[:, rows, p], weights[:, rows, p]
        if name == 'exact':
            positive = before > 0
            assert positive.any() and (out[positive] > 0).all() and np.isfinite(chi2[g, p])
            assert np.array_equal(out[~positive].view(np.uint32), before[~positive].view(np.uint32))
        else:
            assert not out.view(np.uint32).any(), name
            if name == 'constant':
                # (exactly 0, or NaN for a group of a single sample)
                assert not chi2[g, p] > 0.0 and not chi2[g, p] < 0.0
            elif name == 'empty':
                assert np.isnan(chi2[g, p])
            elif name == 'low':
                assert 0.0 < chi2[g, p] < CHI2_RANGE[0]
            else:
                assert CHI2_RANGE[1] < chi2[g, p] < np.inf
    assert sum(counts) == G * P
    assert counts[0] >= ('exact' in marks) and counts[1] >= ('empty' in marks)
