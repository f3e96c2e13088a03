"""The strips of the resident store are (window slack + 1) grid columns wide: the oracle's
store_strip_width, which the exact store tests order by, against the window's slack.  No GPU.

The library has one function for the slack (window_slack, csrc/kimg_window_plan.h, which store.hip,
grid_binned.hip and the window kernels' launches share) and exposes it to Python nowhere, so the 64
widths are pinned here as literals: what store.hip's own strip_width returned for K = 1 .. 64 before
it became window_slack(K) + 1."""
from oracle import kimg_oracle as orc

# K = 1 .. 32: one launch of K taps; K = 33 .. 64: (K + 1) / 2-tap blocks
STRIP_WIDTH = [32, 31, 30, 29, 28, 27, 26, 25, 24, 23, 22, 21, 20, 19, 18, 17,
               16, 15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1,
               16, 16, 15, 15, 14, 14, 13, 13, 12, 12, 11, 11, 10, 10, 9, 9,
               8, 8, 7, 7, 6, 6, 5, 5, 4, 4, 3, 3, 2, 2, 1, 1]


def test_store_strip_width_is_the_window_slack_plus_one():
    assert len(STRIP_WIDTH) == 64
    for K in range(1, 65):
        assert orc.store_strip_width(K) == STRIP_WIDTH[K - 1], K
