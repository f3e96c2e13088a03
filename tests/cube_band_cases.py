"""Long bands for the four newest cube operators (cube_smooth, cube_stats, cube_detect, cube_link): the
cases that test_cube_band_host.py and test_cube_band_gpu.py share, and the assertions that each case
reaches the code path it is there for.  Planes are tiny; the band length is what is under test.

Every ``check_*`` function restates, in a few lines of Python and for the assertion only, the piece of
launch geometry its cases are aimed at (the packing of the radii, the slot count and the workgroup cap
of the statistics, the boxcar's ring, the scan's entries per thread, the filter's tiles) and asserts
from it -- and from the numpy twins' outputs -- that the cases get there.  The host module runs them.

``filled`` patterns come from band_cases; a 1 there reads as a filled channel."""
import numpy as np

import band_cases
import cube_smooth_cases
import detect_cases
import link_cases
import moments_cases

MAX_CHANNELS = 4096
#: scalar; M = 60, the vector form; vector plus tail; where polarizations matter
PLANES = ((1, 3, 5), (1, 5, 12), (1, 1, 61), (3, 3, 5))


def _rng(*seed):
    return np.random.default_rng(list(seed))


# ---- filled ----------------------------------------------------------------------------------------

def single_gaps(C):
    """Single unfilled channels next to seams: 31, 64 and 96 as far as they lie inside the band (never
    its first or last channel).  band_cases' own patterns have no interior gap of one channel:
    single_bits leaves out 31 and 32 (and 63 and 64) together, straddle four channels a seam."""
    filled = np.ones(C, np.uint8)
    for c in (31, 64, 96):
        if 0 < c < C - 1:
            filled[c] = 0
    return filled


def gaps(filled):
    """[(first, length)] of the runs of unfilled channels that have filled channels on both sides."""
    out, c, C = [], 0, len(filled)
    while c < C:
        if filled[c]:
            c += 1
            continue
        end = c
        while end < C and not filled[end]:
            end += 1
        if c > 0 and end < C:
            out.append((c, end - c))
        c = end
    return out


def check_filled():
    """band_cases.self_check for the seam lengths used here, and what the limit mask leaves out."""
    for C in (33, 65, 97, 257, 1025):
        band_cases.self_check(C)
    limit = band_cases.limit_mask(MAX_CHANNELS)
    assert np.flatnonzero(limit == 0).tolist() == [2047, 2048, 4089, 4095]
    words = band_cases.packed(limit)
    assert words[63] == 0x7fffffff and words[64] == 0xfffffffe and words[127] == 0x7dffffff
    assert [g for C in (64, 65, 97, 257) for g in gaps(single_gaps(C))] \
        == [(31, 1), (31, 1), (31, 1), (64, 1), (31, 1), (64, 1), (96, 1)]
    assert gaps(band_cases.single_bits(97)) == [(31, 2), (63, 2)]
    assert gaps(band_cases.straddle(97)) == [(30, 4), (62, 4)]         # (94 .. 96 reach the band's end)


# ---- 1. smoothing ----------------------------------------------------------------------------------

SMOOTH_CHANNELS = (6, 7, 12, 13, 33, 97)
SMOOTH_NOT_FILLED = 31                      # CS_NOT_FILLED
#: what a slot can hold: every radius of the cases, and "not filled"
SMOOTH_CODES = tuple(cube_smooth_cases.RADII) + (SMOOTH_NOT_FILLED,)
SMOOTH_BIG = (7, 16)


def smooth_pack(radius, filled):
    """The kernel argument of cube_smooth.hip: a 5-bit code a channel, six to a 32-bit word."""
    words = [0] * ((len(radius) + 5) // 6)
    for c in range(len(radius)):
        code = int(radius[c]) if filled[c] else SMOOTH_NOT_FILLED
        words[c // 6] |= code << (5 * (c % 6))
    return words


def smooth_code(words, c):
    return (words[c // 6] >> (5 * (c % 6))) & 31


def smooth_tables(C, turn, descending=False):
    """``(radius, filled)``: channel c holds code (c + turn) mod 7 of SMOOTH_CODES (``descending``:
    (turn - c) mod 7), so the seven turns take every slot of every word through every code.  An
    unfilled channel's radius is 0."""
    n = len(SMOOTH_CODES)
    code = [SMOOTH_CODES[((turn - c) if descending else (c + turn)) % n] for c in range(C)]
    filled = np.array([k != SMOOTH_NOT_FILLED for k in code], np.uint8)
    radius = np.array([0 if k == SMOOTH_NOT_FILLED else k for k in code], np.int32)
    return radius, filled


def smooth_short_tables(C):
    """[(name, radius, filled)] of a short band: the seven ascending turns, and descending turn 4, which
    puts "not filled" into slot 5 of word 0 and R = 16 into slot 0 of word 1."""
    out = [(('ascending', turn),) + smooth_tables(C, turn) for turn in range(len(SMOOTH_CODES))]
    if C > 6:
        out.append((('descending', 4),) + smooth_tables(C, 4, descending=True))
    return out


def smooth_limit_tables(swap):
    """``(radius, filled)`` at 4096 channels: R in (0, 1, 2) but for eight channels of R 7 or 16 in the
    first word, the middle word (channels 2046 .. 2051) and the last (4092 .. 4095); of 4094 and 4095
    one is filled (``swap``: 4094) and holds the eighth; some twenty more channels are not filled."""
    C = MAX_CHANNELS
    radius = np.array([(c + c // 6) % 3 for c in range(C)], np.int32)
    filled = np.ones(C, np.uint8)
    filled[[6, 2045, 2052] + list(range(97, C - 8, 197))] = 0
    last, other = (C - 2, C - 1) if swap else (C - 1, C - 2)
    filled[other] = 0
    for c, R in ((0, 16), (5, 7), (2046, 7), (2047, 16), (2051, 16), (C - 4, 16), (C - 3, 7), (last, 7)):
        radius[c] = R
    radius[filled == 0] = 0
    return radius, filled


def smooth_case(C, plane, seed, radius, filled):
    """cube_smooth_cases.make_case with these radii and this ``filled``."""
    cube, _, radius, taps = cube_smooth_cases.make_case(C, plane, seed, radii=list(radius))
    return cube, np.array(filled, np.uint8), radius, taps


def smooth_short_cases(C):
    """[(name, plane, cube, filled, radius, taps)]; the plane rotates with the turn."""
    out = []
    for i, (name, radius, filled) in enumerate(smooth_short_tables(C)):
        plane = PLANES[(i + C) % len(PLANES)]
        out.append(((C,) + name, plane) + smooth_case(C, plane, 10 * C + i, radius, filled))
    return out


def smooth_limit_cases():
    out = []
    for swap, plane in ((False, (1, 5, 12)), (True, (1, 3, 5))):
        radius, filled = smooth_limit_tables(swap)
        out.append(((MAX_CHANNELS, swap), plane) + smooth_case(MAX_CHANNELS, plane, 77 + swap, radius, filled))
    return out


def check_smooth():
    seen = {}                               # (C, word, slot) -> codes
    big_then_unfilled = unfilled_then_big = 0
    for C in SMOOTH_CHANNELS:
        for _, radius, filled in smooth_short_tables(C):
            words = smooth_pack(radius, filled)
            assert len(words) == (C + 5) // 6 and all(w < 2 ** 30 for w in words)
            for c in range(C):
                code = smooth_code(words, c)
                assert code == (radius[c] if filled[c] else SMOOTH_NOT_FILLED)
                seen.setdefault((C, c // 6, c % 6), set()).add(code)
            for w in range(len(words) - 1):
                if w * 6 + 6 < C:
                    a, b = smooth_code(words, 6 * w + 5), smooth_code(words, 6 * w + 6)
                    big_then_unfilled += (a, b) == (16, SMOOTH_NOT_FILLED)
                    unfilled_then_big += (a, b) == (SMOOTH_NOT_FILLED, 16)
        # every slot that the band has in word 0, word 1 and its last word: every code
        last = (C - 1) // 6
        for word in {0, 1, last}:
            for slot in range(6):
                if 6 * word + slot < C:
                    assert seen[(C, word, slot)] == set(SMOOTH_CODES), (C, word, slot)
    assert big_then_unfilled >= 1 and unfilled_then_big >= 1
    # over the bands: all six slots of word 0, word 1 and a last word that is neither
    for word, C in ((0, 6), (1, 12), (1, 13), (16, 97), (5, 33)):
        for slot in range(6 if (word + 1) * 6 <= C else C - 6 * word):
            assert seen[(C, word, slot)] == set(SMOOTH_CODES)
    assert {slot for C in SMOOTH_CHANNELS for slot in range(6) if (C, (C - 1) // 6, slot) in seen} == set(range(6))
    for swap in (False, True):
        radius, filled = smooth_limit_tables(swap)
        words = smooth_pack(radius, filled)
        assert len(words) == 683 and 4 * len(words) + 64 < 4096         # (the arguments fit HIP's 4 KB)
        on = filled != 0
        big = np.flatnonzero(on & np.isin(radius, SMOOTH_BIG))
        assert len(big) == 8 and set(np.unique(radius[on])) == {0, 1, 2, 7, 16}
        assert {int(c) // 6 for c in big} == {0, 341, 682} and 341 == (MAX_CHANNELS // 2) // 6
        assert filled[4094] != filled[4095] and filled[4094] == swap
        assert 10 < (~on).sum() < 40
        for c in (0, 5, 6, 2047, 2048, 4091, 4092, 4094, 4095):
            assert smooth_code(words, c) == (radius[c] if filled[c] else SMOOTH_NOT_FILLED)


# ---- 2. plane statistics ---------------------------------------------------------------------------

STATS_GROUPS = (16, 17, 128, 255, 256, 257, 291)
#: (C, plane, pool_polarizations): C * G takes every value of STATS_GROUPS, twice where a plane of the
#: vector form (W and P * H * W multiples of 4) can give it
STATS_SLOT_CASES = (
    (16, (1, 5, 12), False), (16, (3, 3, 5), True), (17, (1, 5, 12), True), (17, (1, 3, 5), False),
    (128, (1, 5, 12), False), (128, (3, 3, 5), True), (85, (3, 3, 5), False), (255, (1, 5, 12), True),
    (256, (1, 5, 12), False), (256, (1, 1, 61), True), (257, (1, 5, 12), True), (257, (1, 3, 5), False),
    (97, (3, 3, 5), False), (97, (1, 5, 12), True))
STATS_SEAM_CHANNELS = (33, 65, 97)
STATS_MAX_BLOCKS = 8192                     # CST_MAX_BLOCKS
STATS_INIT_THREADS = 4096 * 256             # the threads of cst_init_kernel's largest grid


def stats_slots(groups):
    """cst_slots."""
    return max(1, min(16, 256 // groups))


def stats_cap(active, G):
    """The cap of kimg_cube_stats' workgroup count: below 1 the launch takes one workgroup a group."""
    return STATS_MAX_BLOCKS // (active * G)


def stats_scratch_words(groups):
    """kimg_cube_stats_scratch_bytes / 4: 16 words of state a group, and 2 selects x 2 ranks x slots
    histograms of 256 bins."""
    return groups * 16 + groups * 4 * stats_slots(groups) * 256


def stats_slot_cases():
    """[(name, cube, filled, keywords, region)]"""
    out = []
    for i, (C, plane, pool) in enumerate(STATS_SLOT_CASES):
        values = ('noise_like', 'non_finite', 'three_values')[i % 3]
        cube, filled, region = _stats_case(C, plane, 300 + i, values)
        keywords = dict(estimator=('median_abs', 'mad')[i % 2], pool_polarizations=pool)
        out.append((('slots', C, plane, pool), cube, filled, keywords, region))
    return out


def _stats_case(C, plane, seed, values='noise_like'):
    import cube_stats_cases
    return cube_stats_cases.make_case(C, plane, seed, values, sprinkle=values == 'noise_like')


def stats_seam_cases(C):
    """Every range of moments_cases.seam_ranges under two of band_cases' masks (all five at C = 33,
    which has three ranges); plane, grouping and estimator rotate."""
    out = []
    names = [make.__name__ for make in band_cases.MASKS]
    for i, channels in enumerate(moments_cases.seam_ranges(C)):
        for k in (range(5) if C == 33 else (i % 5, (i + 2) % 5)):
            plane = PLANES[(i + k) % len(PLANES)]
            cube, _, region = _stats_case(C, plane, 1000 * C + 10 * i + k)
            keywords = dict(channels=channels, estimator=('mad', 'median_abs')[(i + k) % 2],
                            pool_polarizations=bool((i + k) % 3))
            out.append((('seam', C, channels, names[k], plane), cube, band_cases.MASKS[k](C), keywords, region))
    return out


STATS_LIMIT_UNFILLED = (0, 31, 32, 2047, 2048, 3000, 4095)


def stats_limit_cases():
    """The three launches at 4096 channels: 12288 groups; 8192 active groups exactly; a range that
    starts one channel past the middle seam."""
    C = MAX_CHANNELS
    filled = np.ones(C, np.uint8)
    filled[list(STATS_LIMIT_UNFILLED)] = 0
    out = []
    cube, _, region = _stats_case(C, (3, 3, 5), 41, 'non_finite')
    out.append((('limit', 'groups'), cube, filled, dict(estimator='mad', pool_polarizations=False), region))
    cube, _, region = _stats_case(C, (2, 3, 4), 42)
    out.append((('limit', 'cap'), cube, np.ones(C, np.uint8),
                dict(estimator='median_abs', pool_polarizations=False), region))
    cube, _, region = _stats_case(C, (1, 5, 12), 43)
    out.append((('limit', 'range'), cube, band_cases.limit_mask(C),
                dict(estimator='median_abs', pool_polarizations=True, channels=(2049, C)), region))
    return out


def stats_quiet_groups(cube_shape, filled, keywords):
    """bool [C][G]: the groups a call leaves as cst_init_kernel made them (count 0, quiet NaN): those
    of channels outside the range and of unfilled ones."""
    C, P = cube_shape[:2]
    first, stop = keywords.get('channels') or (0, C)
    quiet = np.asarray(filled) == 0
    quiet[:first] = True
    quiet[stop:] = True
    G = 1 if keywords.get('pool_polarizations', True) else P
    return np.repeat(quiet.reshape(C, 1), G, axis=1)


def _active(filled, keywords):
    first, stop = keywords.get('channels') or (0, len(filled))
    return int(np.count_nonzero(filled[first:stop]))


def check_stats():
    groups = [C * (1 if pool else plane[0]) for C, plane, pool in STATS_SLOT_CASES]
    assert set(groups) == set(STATS_GROUPS) | {97}                      # (97 pooled: the vector form at C = 97)
    assert [stats_slots(g) for g in STATS_GROUPS] == [16, 15, 2, 1, 1, 1, 1]
    assert {stats_slots(C * (1 if pool else plane[0])) for C, plane, pool in STATS_SLOT_CASES} == {16, 15, 2, 1}
    # both estimators and both kernel forms
    assert {i % 2 for i in range(len(STATS_SLOT_CASES))} == {0, 1}
    assert {plane[2] % 4 == 0 for _, plane, _ in STATS_SLOT_CASES} == {True, False}
    for C in STATS_SEAM_CHANNELS:
        ranges = moments_cases.seam_ranges(C)
        assert {first for first, _ in ranges} == {f for f in (31, 32, 33, 64) if f < C}
        stops = {stop for _, stop in ranges}
        assert {32, 33} <= stops and (C < 65 or {63, 64, 65} <= stops)
        used = {name[3] for name, *_ in stats_seam_cases(C)}
        assert used == {make.__name__ for make in band_cases.MASKS}, C
    (_, a, fa, ka, _), (_, b, fb, kb, _), (_, c, fc, kc, _) = stats_limit_cases()
    assert a.shape == (4096, 3, 3, 5) and stats_cap(_active(fa, ka), 3) < 1
    assert stats_scratch_words(4096 * 3) > STATS_INIT_THREADS           # a second trip of the init loop
    assert all(stats_scratch_words(C * (1 if pool else plane[0])) <= STATS_INIT_THREADS
               for C, plane, pool in STATS_SLOT_CASES)
    assert 50e6 < 4 * stats_scratch_words(4096 * 3) < 52e6
    assert not fa[[2047, 2048, 4095]].any() and 0 < (fa == 0).sum() < 10
    assert b.shape[:2] == (4096, 2) and fb.all() and _active(fb, kb) * 2 == STATS_MAX_BLOCKS
    assert stats_cap(_active(fb, kb), 2) == 1
    assert kc['channels'] == (2049, 4096) and stats_quiet_groups(c.shape, fc, kc).sum() == 2049 + 2


# ---- 3. detection mask -----------------------------------------------------------------------------

BOXCAR_CHANNELS = 257
PRUNE_CHANNELS = (257, 1025)
DT_UNROLL = 4


def prune_minima(C):
    return (2, 31, 32, 33, 64, 255, 256, 257, C) if C > 257 else (2, 31, 32, 33, 64, 255, 256, 257)


def boxcar_slots(width):
    """bx_slots: the rows of the boxcar's ring."""
    slots = 8
    while slots < width - 1 + 2 * 4 - 1:
        slots *= 2
    return slots


def ring_wraps(C, width):
    """How often the ring's row index comes back to 0 over the band."""
    return (C - 1) // boxcar_slots(width)


_ODD_FLOATS = np.array([np.nan, np.inf, -np.inf], np.float32)


def detect_edge_channels(C, width):
    """The channels next to each seam, and the last ``width`` of the band."""
    near = {c for s in band_cases.seams(C) for c in (s - 1, s)}
    return sorted(near | set(range(max(C - width, 0), C)))


def boxcar_case(C, plane, seed, width=31):
    """``(cube, voxel mask)``: detect_cases' sprinkled cube and a random mask with, in every channel
    of detect_edge_channels, a NaN, an Inf or a -Inf in one element and a masked voxel in the next."""
    M = int(np.prod(plane))
    cube = detect_cases.sprinkled_cube(C, plane, seed).reshape(C, M)
    mask = detect_cases.random_mask((C, M), seed + 1, 0.3, values=(1, 1, 2, 255))
    for c in detect_edge_channels(C, width):
        cube[c, c % M] = _ODD_FLOATS[c % 3]
        cube[c, (c + 1) % M] = np.float32(1.5 + c % 7)
        mask[c, c % M] = 0
        mask[c, (c + 1) % M] = (1, 2, 255)[c % 3]
    return cube.reshape((C,) + tuple(plane)), mask.reshape((C,) + tuple(plane))


def boxcar_options():
    """[(width, with_mask, blank)]: every width with every option."""
    return [(width, with_mask, blank) for width in detect_cases.WIDTHS for with_mask in (False, True)
            for blank in (False, True)]


def boxcar_limit_options():
    return [(1, False, False), (1, True, True), (31, False, True), (31, True, False)]


PRUNE_PLACEMENTS = ('at 0', 'to the end', 'from a seam', 'to a seam', 'from 4k - 1', 'from 4k + 1',
                    'to 4k - 1', 'to 4k + 1')
PRUNE_VARIANTS = ('ones', 'first', 'middle', 'last', 'at min - 1', 'after min', 'none is 1')


def _prune_start(C, length, placement):
    """The first channel of a run of ``length`` at ``placement``, or None where the band has no room."""
    if length < 1 or length > C:
        return None
    top = (C - 2) // 4 * 4                  # a multiple of DT_UNROLL below the last channel
    seam = -(-length // 32) * 32            # the first seam a run from 0 can end on ...
    if seam == length:
        seam += 32                          # ... without starting at 0
    start = {'at 0': 0, 'to the end': C - length, 'from a seam': 32 if length < 64 else 64,
             'to a seam': seam - length, 'from 4k - 1': 3, 'from 4k + 1': 5,
             'to 4k - 1': top - length, 'to 4k + 1': top + 2 - length}[placement]
    if start < 0 or start + length > C:
        return None
    if placement not in ('at 0', 'to the end') and (start == 0 or start + length == C):
        return None
    return start


def prune_columns(C, min_channels):
    """[(length, placement, variant, start)] of the one-run columns of the prune mask."""
    out = []
    for length in (min_channels - 1, min_channels, min_channels + 1):
        for placement in PRUNE_PLACEMENTS:
            start = _prune_start(C, length, placement)
            if start is None:
                continue
            for variant in PRUNE_VARIANTS:
                if variant == 'at min - 1' and length < min_channels:
                    continue
                if variant == 'after min' and length <= min_channels:
                    continue
                out.append((length, placement, variant, start))
    return out


def prune_mask(C, min_channels):
    """uint8 [C][M], built element by element: a column a run of prune_columns -- bytes 1 but where the
    variant puts a 2 or a 255 --, then eight columns of runs of min - 1, min and min + 1 channels one
    after the other with a channel between them, the first run starting at channel 0 .. 3 and a byte
    in four not 1; an empty and a full column; M made a multiple of 4 with empty columns."""
    columns = prune_columns(C, min_channels)
    M = -(-(len(columns) + 10) // 4) * 4
    mask = np.zeros((C, M), np.uint8)
    for j, (length, placement, variant, start) in enumerate(columns):
        run = np.ones(length, np.uint8)
        if variant == 'first':
            run[0] = 2
        elif variant == 'middle':
            run[length // 2] = 255
        elif variant == 'last':
            run[-1] = 2
        elif variant == 'at min - 1':
            run[min_channels - 1] = 255
        elif variant == 'after min':
            run[min_channels:] = 2
        elif variant == 'none is 1':
            run[:] = (2, 255)[j % 2]
        mask[start:start + length, j] = run
    rng = _rng(C, min_channels)
    for k in range(8):
        j = len(columns) + k
        c, turn = k % 4, k
        while c < C:
            length = max(min_channels - 1 + turn % 3, 1)
            run = rng.choice(np.array([1, 1, 1, 2 if k < 4 else 255], np.uint8), length)
            mask[c:c + length, j] = run[:C - c]
            c += length + 1
            turn += 1
    mask[:, len(columns) + 8] = 1
    return mask


def prune_walks(mask, min_channels):
    """``(clear, rewrite)``: the most channels dt_prune_kernel's two back-writing loops walk in any
    element of this mask -- a run below min_channels is cleared whole; a run that reaches min_channels
    with a byte that is not 1 among its first min_channels - 1 has those rewritten."""
    C, M = mask.shape
    clear = rewrite = 0
    for j in range(M):
        on = np.flatnonzero(np.diff(np.r_[0, mask[:, j] != 0, 0]))
        for start, end in zip(on[::2], on[1::2]):
            if end - start < min_channels:
                clear = max(clear, int(end - start))
            elif (mask[start:start + min_channels - 1, j] != 1).any():
                rewrite = max(rewrite, min_channels - 1)
    return clear, rewrite


def check_prune(C, min_channels, mask, pruned):
    """From the mask and the twin's output: every length that fits sits at every placement that has
    room for it (all of them up to min_channels = 64), the odd bytes are where the variants say, short
    runs are gone and long ones all 1."""
    columns = prune_columns(C, min_channels)
    placed = {(length, placement) for length, placement, _, _ in columns}
    for length in (min_channels - 1, min_channels, min_channels + 1):
        for placement in PRUNE_PLACEMENTS:
            fits = _prune_start(C, length, placement) is not None
            assert ((length, placement) in placed) == fits
            assert fits or length < 1 or min_channels > 64, (C, min_channels, length, placement)
    for j, (length, placement, variant, start) in enumerate(columns):
        column, end = mask[:, j], start + length
        assert np.count_nonzero(column) == length and column[start:end].all()
        assert {'at 0': start == 0, 'to the end': end == C, 'from a seam': start % 32 == 0 and start > 0,
                'to a seam': end % 32 == 0 and end < C, 'from 4k - 1': start % DT_UNROLL == 3,
                'from 4k + 1': start % DT_UNROLL == 1, 'to 4k - 1': (end - 1) % DT_UNROLL == 3,
                'to 4k + 1': (end - 1) % DT_UNROLL == 1}[placement], (C, min_channels, placement, start)
        odd = np.flatnonzero(column[start:end] != 1).tolist()
        want = {'ones': [], 'first': [0], 'middle': [length // 2], 'last': [length - 1],
                'at min - 1': [min_channels - 1], 'after min': list(range(min_channels, length)),
                'none is 1': list(range(length))}[variant]
        assert odd == want, (C, min_channels, variant)
        assert pruned[:, j].tolist() == ((column != 0) * (length >= min_channels)).tolist(), \
            (C, min_channels, length, placement, variant)
    variants = {(length >= min_channels, variant) for length, _, variant, _ in columns}
    assert {v for long, v in variants if long} == set(PRUNE_VARIANTS) or min_channels + 1 > C
    assert set(np.unique(pruned)) <= {0, 1}
    clear, rewrite = prune_walks(mask, min_channels)
    assert clear == min_channels - 1 and rewrite == min_channels - 1
    return clear, rewrite


def threshold_case(C, filled, seed, polarity):
    """``(work, mask, sigma [C][3])`` on the plane (3, 3, 5): in the channels next to each seam and in
    the last one, a group's sigma puts the cut between the two middle ones of its finite voxels that
    the mask has not set yet (as the polarity reads them), so that it decides voxels both ways;
    elsewhere detect_cases.sigma_table."""
    plane = (3, 3, 5)
    work = detect_cases.sprinkled_cube(C, plane, seed)
    mask = detect_cases.random_mask(work.shape, seed + 1, 0.2, values=(1, 2, 255))
    sigma = detect_cases.sigma_table(C, 3, seed + 2)
    for c in threshold_rows(C, filled):
        for g in range(3):
            v = work[c, g][np.isfinite(work[c, g]) & (mask[c, g] == 0)].astype(np.float64)
            s = np.unique({'positive': v, 'negative': -v, 'both': np.abs(v)}[polarity])
            sigma[c, g] = np.float32(0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2]) / THRESHOLD)
    return work, mask, sigma


THRESHOLD = 1.25


def threshold_rows(C, filled):
    """The filled channels nearest below and above every seam, and the last filled one."""
    on = np.flatnonzero(filled)
    rows = {int(on[-1])}
    for s in band_cases.seams(C):
        rows.update(int(c[0]) for c in (on[on < s][-1:], on[on >= s][:1]) if len(c))
    return sorted(rows)


def check_threshold(C, filled, work, mask, sigma, result, polarity):
    """In every row of threshold_rows, every group: a voxel set by the call and a finite one left."""
    rows = threshold_rows(C, filled)
    assert rows[-1] == np.flatnonzero(filled)[-1] and len(rows) >= 2 * len(band_cases.seams(C)) - 1
    for c in rows:
        for g in range(3):
            new = (result[c, g] == 1) & (mask[c, g] == 0)
            left = (result[c, g] == 0) & np.isfinite(work[c, g])
            assert new.any() and left.any(), (C, c, g, polarity)
    assert np.array_equal(result[filled == 0], mask[filled == 0])


def check_detect():
    for width in detect_cases.WIDTHS:
        assert ring_wraps(BOXCAR_CHANNELS, width) >= 4
    assert boxcar_slots(31) == 64 and ring_wraps(BOXCAR_CHANNELS, 31) == 4
    assert boxcar_slots(1) == 8 and ring_wraps(BOXCAR_CHANNELS, 1) == 32
    assert [boxcar_slots(w) for w in detect_cases.WIDTHS] == [8, 16, 16, 32, 64]
    names = {name for name, _ in band_cases.masks(BOXCAR_CHANNELS)}
    assert names == {make.__name__ for make in band_cases.MASKS}
    # gaps longer than every window, and outputs that start after a full ring of skipped channels
    assert max(n for _, n in gaps(band_cases.alternate_words(BOXCAR_CHANNELS))) == 32 > max(detect_cases.WIDTHS)
    assert not band_cases.word0_empty(BOXCAR_CHANNELS)[:32].any()
    cube, mask = boxcar_case(BOXCAR_CHANNELS, (1, 3, 5), 1)
    for c in detect_edge_channels(BOXCAR_CHANNELS, 31):
        assert (~np.isfinite(cube[c])).any() and (mask[c][np.isfinite(cube[c])] != 0).any()
    assert set(range(226, 257)) | {31, 32, 223, 224} <= set(detect_edge_channels(BOXCAR_CHANNELS, 31))
    assert {w for w, _, _ in boxcar_options()} == set(detect_cases.WIDTHS) and len(boxcar_options()) == 20
    assert {w for w, _, _ in boxcar_limit_options()} == {1, 31}


# ---- 4. linking ------------------------------------------------------------------------------------

LINK_SEAM_CHANNELS = (64, 65, 97, 257)
LINK_SEAM_PLANES = ((3, 3, 5), (1, 5, 12))
LINK_REACHES = tuple((xy, z) for z in (1, 2, 3) for xy in (0, 1))
LINK_FILLED = (band_cases.single_bits, band_cases.straddle, single_gaps)
LK_CHUNK = 1024
LK_SCAN_THREADS = 1024
#: (C, plane): 1100, 2050 and 4096 workgroups, and two a channel
LINK_SCAN_SHAPES = ((1100, (1, 1, 3)), (2050, (1, 1, 5)), (4096, (1, 1, 1)), (4096, (1, 25, 41)))


def column_pixel(plane, p):
    """(y, x) of polarization p's column."""
    return p % plane[1], (2 * p + 1) % plane[2]


def link_seam_mask(C, plane, seed):
    """A random mask of a tenth, values 1, 2 and 255, with one pixel of every polarization set in
    every channel."""
    mask = link_cases.random_mask((C,) + tuple(plane), seed, 0.1, values=(1, 1, 2, 255))
    for p in range(plane[0]):
        y, x = column_pixel(plane, p)
        mask[:, p, y, x] = (1, 2, 255)[p % 3]
    return mask


def link_seam_cases(C):
    """[(name, mask, cube, filled, reach, minima)]: both planes under every pattern of LINK_FILLED and
    every reach of LINK_REACHES; integer and Gaussian cubes alternate."""
    out = []
    for i, plane in enumerate(LINK_SEAM_PLANES):
        mask = link_seam_mask(C, plane, C + i)
        shape = mask.shape
        cubes = (link_cases.integer_cube(shape, C + i), link_cases.gaussian_cube(shape, C + i))
        for k, make in enumerate(LINK_FILLED):
            for n, reach in enumerate(LINK_REACHES):
                minima = ((1, 1, 1), (3, 1, 1), (1, 1, 2), (2, 2, 1))[(k + n) % 4]
                out.append(((C, plane, make.__name__, reach), mask, cubes[(i + k + n) % 2], make(C), reach, minima))
    return out


def column_pieces(labels, filled, plane, p):
    """The distinct sources along polarization p's column."""
    y, x = column_pixel(plane, p)
    return len(set(labels[filled != 0, p, y, x].tolist()))


def check_link_seam(name, labels, filled):
    """From link_host's labels: the column is split exactly at the gaps of ``filled`` that are as long
    as reach_z or longer.  Returns (pieces, gaps)."""
    C, plane, _, (_, reach_z) = name
    between = gaps(filled)
    want = 1 + sum(1 for _, length in between if length >= reach_z)
    for p in range(plane[0]):
        assert column_pieces(labels, filled, plane, p) == want, (name, p)
    return want, len(between)


def check_link_seams(results):
    """``results``: {name: (pieces, gaps)} of every seam case.  A single unfilled channel splits the
    column under reach_z = 1 and is bridged under 2; single_bits' gaps of two channels are bridged
    under 3 only; straddle's gaps of four never."""
    for (C, plane, pattern, (xy, z)), (pieces, between) in results.items():
        assert between >= 1, (C, pattern)
        if pattern == 'single_gaps':
            assert pieces == (between + 1 if z == 1 else 1)
        elif pattern == 'single_bits':
            assert pieces == (1 if z == 3 else between + 1)
        else:
            assert pieces == between + 1
    assert {name[:2] for name in results} == {(C, plane) for C in LINK_SEAM_CHANNELS for plane in LINK_SEAM_PLANES}


def scan_entries(blocks):
    """lk_scan_kernel: entries a thread, the threads that have any, and the size of the last one's run."""
    per = -(-blocks // LK_SCAN_THREADS)
    busy = -(-blocks // per)
    return per, busy, blocks - per * (busy - 1)


def link_blocks(C, plane):
    return C * -(-int(np.prod(plane)) // LK_CHUNK)


def middle_unfilled(C):
    """Unfilled: the two channels below and the two above the seam nearest the middle of the band."""
    seam = (C // 2 + 16) // 32 * 32
    filled = np.ones(C, np.uint8)
    filled[seam - 2:seam + 2] = 0
    return filled


def link_scan_masks(C, plane, seed):
    """``(all set, sparse)``: the sparse one has some 400 voxels set at random and polarization 0's
    column through every channel."""
    shape = (C,) + tuple(plane)
    sparse = link_cases.random_mask(shape, seed, min(0.2, 400.0 / np.prod(shape)), values=(1, 2, 255))
    y, x = column_pixel(plane, 0)
    sparse[:, 0, y, x] = 1
    return np.ones(shape, np.uint8), sparse


def link_scan_cases(C, plane):
    """[(name, mask, filled, reach)]: all set at reach (0, 0) and sparse at reach (1, 1), every channel
    filled and with the middle seam's neighbours unfilled."""
    every, sparse = link_scan_masks(C, plane, C + plane[2])
    return [(('all set', 'filled'), every, np.ones(C, np.uint8), (0, 0)),
            (('sparse', 'filled'), sparse, np.ones(C, np.uint8), (1, 1)),
            (('all set', 'middle'), every, middle_unfilled(C), (0, 0)),
            (('sparse', 'middle'), sparse, middle_unfilled(C), (1, 1))]


def check_link_scan_case(name, mask, filled, labels, N0):
    """From link_host's output."""
    C, plane = mask.shape[0], mask.shape[1:]
    on = filled != 0
    if name[0] == 'all set':
        # every voxel its own source; the labels ascend with the dense index
        want = np.zeros(mask.shape, np.int32)
        want[on] = np.arange(1, int(on.sum()) * int(np.prod(plane)) + 1, dtype=np.int32).reshape((-1,) + plane)
        assert N0 == int(on.sum()) * int(np.prod(plane)) and np.array_equal(labels, want), name
    else:
        y, x = column_pixel(plane, 0)
        column = labels[:, 0, y, x]
        if name[1] == 'filled':
            # one source from the first channel to the last
            assert column[0] > 0 and (column == column[0]).all(), name
        else:
            assert len(set(column[on].tolist())) == 2 and not column[~on].any(), name
    return N0


def check_link_scan():
    shapes = {shape: scan_entries(link_blocks(*shape)) for shape in LINK_SCAN_SHAPES}
    assert shapes[LINK_SCAN_SHAPES[0]] == (2, 550, 2)           # the upper half of the threads empty
    assert shapes[LINK_SCAN_SHAPES[1]] == (3, 684, 1)           # one thread with a single entry
    assert shapes[LINK_SCAN_SHAPES[2]] == (4, 1024, 4)
    assert shapes[LINK_SCAN_SHAPES[3]][0] >= 8 and link_blocks(*LINK_SCAN_SHAPES[3]) == 2 * 4096
    assert int(np.prod(LINK_SCAN_SHAPES[3][1])) == 1025         # the smallest plane above 1024 elements
    for C, _ in LINK_SCAN_SHAPES:
        filled = middle_unfilled(C)
        seam = int(np.flatnonzero(filled == 0)[2])
        assert seam % 32 == 0 and abs(seam - C // 2) <= 16 and (filled == 0).sum() == 4


FILTER_SHAPE = (160, 1, 5, 12)
FILTER_MINIMA = ((2, 1, 1), (1, 1, 3))
LK_TILE = 1024


def filter_runs_mask():
    """Runs of 1 .. 4 channels along the channel axis with a channel between them, in every pixel of
    FILTER_SHAPE, out of step from pixel to pixel: at reach (0, 1) every run is a source."""
    C, _, H, W = FILTER_SHAPE
    mask = np.zeros(FILTER_SHAPE, np.uint8)
    flat = mask.reshape(C, H * W)
    for j in range(H * W):
        c, turn = j % 3, j
        while c < C:
            length = 1 + turn % 4
            flat[c:c + length, j] = (1, 2, 255)[turn % 3]
            c += length + 1
            turn += 1
    return mask


def filter_exact_mask(N0):
    """Exactly N0 voxels of (41, 1, 5, 5), every one its own source at reach (0, 0)."""
    mask = np.ones(41 * 25, np.uint8)
    mask[N0:] = 0
    return mask.reshape(41, 1, 5, 5)


def filter_keep(table, minima):
    t = table
    return ((t['voxels'] >= minima[0]) & (t['x1'] - t['x0'] + 1 >= minima[1])
            & (t['y1'] - t['y0'] + 1 >= minima[1]) & (t['c1'] - t['c0'] + 1 >= minima[2]))


def check_filter_runs(table):
    """From measure_host's table of filter_runs_mask: N0 > 2048, and under both minima 1024 < N < N0
    with kept and dropped rows in every tile of 1024."""
    N0 = len(table)
    assert N0 > 2 * LK_TILE
    for minima in FILTER_MINIMA:
        keep = filter_keep(table, minima)
        assert LK_TILE < keep.sum() < N0, (minima, int(keep.sum()))
        for base in range(0, N0, LK_TILE):
            tile = keep[base:base + LK_TILE]
            assert tile.any() and not tile.all(), (minima, base)
            # interleaved: never a long stretch of one kind
            change = np.flatnonzero(np.diff(tile.astype(np.int8)))
            assert len(change) >= len(tile) // 16, (minima, base)
    return N0
