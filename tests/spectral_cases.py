"""What test_spectral_gpu.py runs on the device, kept apart from it so that test_spectral_host.py can
check, without a device, that these lists reach every form of csrc/spectral.hip and every branch of
its loops: the filters, the shape lists, the (length, offset, step) cases of the C entry point, the
random block both files draw, and the contract of include/kimg.h ("Spectral filter") once more in
float64, for parameters that spectral.SpectralParameters cannot express."""
import numpy as np

HANNING = (0.25, 0.5, 0.25)
FIVE = (0.1, 0.2, 0.4, 0.2, 0.1)
#: dyadic, so that a coverage of exactly one half is an ascending float64 sum: 1/4 + 3/16 + 1/16
SEVEN = (1 / 16, 1 / 8, 3 / 16, 1 / 4, 3 / 16, 1 / 8, 1 / 16)
NINE = (0.02, 0.05, 0.11, 0.17, 0.3, 0.17, 0.11, 0.05, 0.02)
#: SF_CHUNK of csrc/spectral.hip: output channels per blockIdx.y (test_spectral_host.py compares)
CHUNK = 64

#: (C_in, taps, bin); the last two: two chunks of output channels and five more, so that windows
#: straddle both chunk seams.  Run on every plane, with a second stream and repeated calls.
SHAPES = [
    (1, HANNING, 1), (2, HANNING, 1), (3, HANNING, 1), (7, (1.0,), 2), (7, HANNING, 2),
    (64, (1.0,), 64), (9, NINE, 1), (3 * (2 * CHUNK + 5) + 1, HANNING, 3), (2 * CHUNK + 5, FIVE, 1),
]

#: (C_in, taps, bin), on three planes: what the control flow of every form needs beyond SHAPES.
#: R is the number of outputs of one round of a sliding form.
FORM_SHAPES = [
    # sliding, L = 3 (R = 6)
    (6, HANNING, 1),                    # one exact round, no prefetch
    (7, HANNING, 1),                    # the prefetch is taken once, then a round of 1
    (12, HANNING, 1),                   # two exact rounds: a prefetch and no partial round
    (13, HANNING, 1),                   # two prefetches, then a round of 1
    (CHUNK, HANNING, 1),                # one full chunk: ten rounds and a last one of 4
    (2 * CHUNK + 5, HANNING, 1),        # two seams, the halo re-read at o_begin = 64 and 128, a
                                        # last chunk shorter than R
    # sliding, L = 5 (R = 5)
    (4, FIVE, 1),                       # the band is shorter than the window: clipped at both ends
    (5, FIVE, 1),                       # one exact round
    (6, FIVE, 1),                       # a prefetch, then a round of 1
    # sliding, L = 7 (R = 7)
    (3, SEVEN, 1),                      # band shorter than the window
    (7, SEVEN, 1),                      # one exact round
    (8, SEVEN, 1),                      # a prefetch, then a round of 1
    (2 * CHUNK + 5, SEVEN, 1),          # two seams; chunks end in a round of 1, the last in one of 5
    # sliding, L = 9 (R = 9)
    (4, NINE, 1),                       # band shorter than the window
    (10, NINE, 1),                      # a prefetch, then a round of 1
    (2 * CHUNK + 5, NINE, 1),           # two seams; chunks end in a round of 1, the last in one of 5
    # disjoint
    (3 * (2 * CHUNK + 5) + 2, (1.0,), 3),   # length 3, two seams, two input channels left over
                                            # that no output may read
    (5 * 70, (1.0,), 5),                # length 5 (one unroll group and one more), one seam
    (64 * 66, (1.0,), 64),              # the largest bin, across a seam
    # window
    (5 * (2 * CHUNK + 5) + 3, NINE, 5),     # length 13: three unroll groups and one more, two seams
    (64 * 66 + 3, NINE, 64),            # length 72, the maximum, across a seam
    (64 * 2, HANNING, 64),              # length 66: sixteen unroll groups and two more
    (2 * 70 + 1, SEVEN, 2),             # length 8: no remainder against the unroll, one seam
    (3, HANNING, 2),                    # length 4 on three channels: band shorter than the window
]
#: (N, Q) for FORM_SHAPES: a whole wave and one lane (large enough for the hand-made samples), partial
#: workgroups with three polarizations, one element
FORM_PLANES = [(65, 1), (257, 3), (1, 1)]

#: the C entry point called directly: input channels, and (length, offset, step)
ABI_CHANNELS = 2 * CHUNK + 5
ABI_CASES = (
    # the sliding forms at the first, the middle and the last offset
    [(L, offset, 1) for L in (3, 5, 7, 9) for offset in (0, L // 2, L - 1)]
    # even lengths at step 1: the window form as Python never calls it
    + [(L, offset, 1) for L in (2, 4, 6, 8) for offset in (0, L - 1)]
    + [(7, 0, 3), (7, 3, 3), (7, 6, 3)]
    # the disjoint form as a copy that handles flags
    + [(1, 0, 1)]
)


def random_block(rng, C, N, Q):
    """complex64 visibilities of a few units and float32 weights U(0.5, 2) with 20 % zeros, [C][N][Q]."""
    vis = ((rng.normal(size=(C, N, Q)) + 1j * rng.normal(size=(C, N, Q))) * 3.0).astype(np.complex64)
    weights = rng.uniform(0.5, 2.0, (C, N, Q)).astype(np.float32)
    weights[rng.random((C, N, Q)) < 0.2] = 0.0
    return vis, weights


def window(length, offset, step, o, C_in):
    """(i, c) of the inputs of output o that lie inside the band."""
    return [(i, o * step - offset + i) for i in range(length) if 0 <= o * step - offset + i < C_in]


def contract_double(vis, weights, g, offset, step, min_sum, C_out):
    """include/kimg.h, "Spectral filter", output by output in float64 for any (g, offset, step):
    (vis complex128 and weights float64 before their one rounding, kept bool), all [C_out][N][Q] and
    0 where not kept -- what spectral.filter_host_double returns."""
    C_in = vis.shape[0]
    plane = vis.shape[1:]
    usable = (weights > 0) & np.isfinite(vis.real) & np.isfinite(vis.imag)
    out = np.zeros((C_out,) + plane, np.complex128)
    new_weights = np.zeros((C_out,) + plane, np.float64)
    kept = np.zeros((C_out,) + plane, bool)
    for o in range(C_out):
        cov, S1, S2, Nr, Ni = (np.zeros(plane, np.float64) for k in range(5))
        for i, c in window(len(g), offset, step, o, C_in):
            u = usable[c]
            w = weights[c, u].astype(np.float64)
            v = vis[c, u].astype(np.complex128)
            cov[u] += g[i]
            S1[u] += g[i] * w
            S2[u] += g[i] * (g[i] * w)
            Nr[u] += g[i] * (w * v.real)
            Ni[u] += g[i] * (w * v.imag)
        k = cov >= min_sum
        kept[o] = k
        out[o].real[k] = Nr[k] / S1[k]
        out[o].imag[k] = Ni[k] / S1[k]
        new_weights[o, k] = (S1[k] * S1[k]) / S2[k]
    return out, new_weights, kept
