"""Bands longer than one word of the per-channel bit mask, shared by the host and device tests of the
operators that walk the channel axis inside one thread (continuum fit, statwt, flagger, moments): the
channel counts, and masks whose set and clear bits sit on the seams between the mask's 32-bit words.

A mask here is a uint8 array [C], 1 for a fit (searched) channel and 0 for a line (protected) one, as
the operators' ``fit_mask=`` takes it.  Bit c & 31 of word c >> 5 of the packed mask is mask[c]."""
import numpy as np

WORD = 32
#: one word exactly, one channel into the second, two words, one channel into the third, and a
#: fourth word that holds a single channel
SEAM_CHANNELS = (32, 33, 64, 65, 97)
#: 33 words, the last of them with a single channel
LONG_CHANNELS = 1025
CHANNELS = SEAM_CHANNELS + (LONG_CHANNELS,)
#: (rows, polarizations): a partial second wave, and a second workgroup
PLANES = ((65, 1), (257, 2))


def seams(C):
    """The first channel of every word after word 0."""
    return list(range(WORD, C, WORD))


def words(C):
    return (C + WORD - 1) // WORD


def straddle(C):
    """Line channels s - 2 .. s + 1 around every seam s."""
    mask = np.ones(C, np.uint8)
    for s in seams(C):
        mask[s - 2:s + 2] = 0
    return mask


def word0_empty(C):
    """Every channel of word 0 a line channel, the rest fit channels."""
    mask = np.ones(C, np.uint8)
    mask[:WORD] = 0
    return mask


def last_only_high(C):
    """Fit channels only in the last (partial) word and the one before it."""
    mask = np.zeros(C, np.uint8)
    mask[max(words(C) - 2, 0) * WORD:] = 1
    return mask


def alternate_words(C):
    """Even words fit, odd words line."""
    return ((np.arange(C) // WORD) % 2 == 0).astype(np.uint8)


def single_bits(C):
    """Only channels 31, 32, 63, 64 and C - 1 line channels, as far as they exist."""
    mask = np.ones(C, np.uint8)
    for c in (31, 32, 63, 64, C - 1):
        if c < C:
            mask[c] = 0
    return mask


MASKS = (straddle, word0_empty, last_only_high, alternate_words, single_bits)


def masks(C, least=1):
    """[(name, mask)] for a band of C channels: every mask of MASKS that leaves at least ``least`` fit
    channels (order + 1 for a fit of that order; 1 for an operator that only needs a channel)."""
    out = [(make.__name__, make(C)) for make in MASKS]
    return [(name, mask) for name, mask in out if int(mask.sum()) >= least]


def limit_mask(C):
    """The mask of the launch at the operator's longest band: its only line channels are the two on
    either side of the middle seam (8191 and 8192 of 16384) and two in the last word, the band's last
    channel one of them."""
    mask = np.ones(C, np.uint8)
    mask[[C // 2 - 1, C // 2, C - 7, C - 1]] = 0
    return mask


def packed(mask):
    """The mask as the host code packs it: uint32 words, bit c & 31 of word c >> 5."""
    mask = np.asarray(mask) != 0
    out = np.zeros(words(len(mask)), np.uint32)
    for c in np.flatnonzero(mask):
        out[c >> 5] |= np.uint32(1) << np.uint32(c & 31)
    return out


def self_check(C):
    """The masks of a band of C channels together put a set bit and a clear bit at bit 31 of a word and
    at bit 0 of the next word, for every seam of the band, and a set and a clear bit into the band's
    last word.  (A band of one word has no seam: bit 31 of its only word is checked.)"""
    all_words = [packed(mask) for _, mask in masks(C, least=0)]
    assert len(all_words) == len(MASKS)

    def both(word, bit):
        values = {int(w[word] >> np.uint32(bit)) & 1 for w in all_words}
        return values == {0, 1}
    assert both(0, 31), (C, 'bit 31 of word 0')
    for s in seams(C):
        assert both((s >> 5) - 1, 31), (C, s, 'bit 31 before the seam')
        assert both(s >> 5, 0), (C, s, 'bit 0 after the seam')
    last = words(C) - 1
    in_last = range(last * WORD, C)
    assert any(mask[c] for _, mask in masks(C, least=0) for c in in_last), (C, 'a set bit in the last word')
    assert any(not mask[c] for _, mask in masks(C, least=0) for c in in_last), (C, 'a clear bit there')
    # the packing itself: the bits that were put in come out, and nothing lies past the band
    for _, mask in masks(C, least=0):
        w = packed(mask)
        back = [(int(w[c >> 5]) >> (c & 31)) & 1 for c in range(C)]
        assert back == mask.tolist()
        assert int(w[last]) >> (((C - 1) & 31) + 1) == 0
