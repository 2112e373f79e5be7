"""CPU: the n-tuple deep search of g2048_device.h -- the header the kernels are compiled from -- built for the host
(tests/host_ntuple_deep/deep_check.cpp, g++).  ntuple_search_root<3> against the pure-Python reference
tests/ntuple_search_ref.py, and the split of ntuple_deep_search_kernel (root, expand, scan, leaves, fold, finish over the
table the kernel keeps in LDS) run by P simulated lanes against ntuple_search_root at depths 2 and 3.  Every case shows from
the reference's own trace (never from the code under test) that its input reaches the edge it names."""
import numpy as np
import pytest

import ntuple_ref as ref
import ntuple_search_ref as sref
from analysis_helpers import ONE_LEGAL, TERMINAL, mixed_boards
from ntuple_deep_helpers import (HUGE, MERGING, chance_sums, host_root, host_split, load_host_deep, mixed_net, near_full, raw_desc,
                                 reference_search, staged_net, values_of)
from ntuple_helpers import TUPLES_8x4, TUPLES_17x4, random_net
from ntuple_mixed_helpers import near_full_12
from ntuple_search_helpers import PAIR_ONLY, WIDE_FANS, assert_search_equal

LANES = (1, 64, 256)


@pytest.fixture(scope="module")
def hd():
    return load_host_deep()


def assert_split_equals_root(lib, boards, depth, net, where):
    want = host_root(lib, boards, depth, net)
    for P in LANES:
        got, items, units = host_split(lib, boards, depth, net, P)
        assert_search_equal(got, want, boards, f"{where}, depth {depth}, {P} lanes")
    return want, items, units


@pytest.mark.parametrize("max_empty, tuples", [(1, "1x4"), (2, "1x4"), (1, "2x6"), (2, "2x6")])
def test_depth_3_root_equals_the_reference(hd, max_empty, tuples):
    boards, net, want3, want2, trace = near_full(max_empty, tuples)
    assert trace.chance > 4000 and trace.negative_inexact > 200 and trace.terminal_children > 30
    assert (want3[0] != want2[0]).any(), "inputs: the third ply changes a move"
    assert_search_equal(host_root(hd, boards, 3, net), want3, boards, "depth 3")
    assert_search_equal(host_root(hd, boards, 2, net), want2, boards, "depth 2")
    # the kernel's split on the same boards
    for P in LANES:
        assert_search_equal(host_split(hd, boards, 3, net, P)[0], want3, boards, f"split, {P} lanes")


def test_depth_3_named_boards(hd):
    """PAIR_ONLY (a child with no legal move right below the root), ONE_LEGAL (three illegal root directions) and TERMINAL."""
    net = random_net(TUPLES_8x4[:1], 32)
    boards = np.concatenate([PAIR_ONLY, TERMINAL])
    trace = sref.Trace()
    want = sref.search_batch(boards, 3, net, trace)
    assert trace.terminal_children >= 2 and (want[1][1] == sref.ILLEGAL).all() and want[0][1] == 0
    assert (want[1][0] == sref.ILLEGAL).sum() == 2
    assert_search_equal(host_root(hd, boards, 3, net), want, boards, "depth 3")
    assert_split_equals_root(hd, boards, 3, net, "named")
    # ONE_LEGAL has four empty cells after its one move: the reference affords depth 3 there too
    one = host_root(hd, ONE_LEGAL, 3, net)
    assert_search_equal(one, sref.search_batch(ONE_LEGAL, 3, net), ONE_LEGAL, "one legal, depth 3")
    assert one[0][0] == 2 and (one[1][0, [0, 1, 3]] == sref.ILLEGAL).all() and one[1][0, 2] != sref.ILLEGAL
    assert_split_equals_root(hd, ONE_LEGAL, 3, net, "one legal")
    assert_search_equal(host_split(hd, ONE_LEGAL, 2, net, 256)[0], sref.search_batch(ONE_LEGAL, 2, net), ONE_LEGAL, "one legal, depth 2")


def test_split_depth_2_mixed_boards(hd):
    net = random_net(TUPLES_17x4, 33)
    boards = np.concatenate([mixed_boards(40, 31), ONE_LEGAL, TERMINAL, PAIR_ONLY])
    (act, val), items, units = assert_split_equals_root(hd, boards, 2, net, "mixed boards")
    legal = val != sref.ILLEGAL
    assert len(set(act.tolist())) == 4 and (~legal).any() and (val[legal] < 0).any() and (val[legal] > 0).any()
    # from the definition: a board's level-1 items are the 2 E of its legal afterstates
    want_items = [sum(2 * sum(x == 0 for x in a) for a, _, ok in (ref.move(ref.plain(b), d) for d in range(4)) if ok) for b in boards]
    assert items.tolist() == want_items and max(want_items) > 64 and 0 in want_items
    assert units.max() > 256, "inputs: some board has more work units than the kernel has lanes"


def test_split_depth_3_wide_fan(hd):
    """One sparse board at depth 3: 30 items in a direction, thousands of work units."""
    net = random_net(TUPLES_8x4[:1], 34)
    board = WIDE_FANS[1:2]
    assert max(2 * sum(x == 0 for x in ref.move(ref.plain(board[0]), d)[0]) for d in range(4)) == 30
    _, items, units = assert_split_equals_root(hd, board, 3, net, "wide fan")
    assert items[0] >= 60 and units[0] > 4 * 256


def test_split_depth_2_all_wide_fans(hd):
    net = random_net(TUPLES_8x4[:1], 35)
    (_, val), items, _ = assert_split_equals_root(hd, WIDE_FANS, 2, net, "wide fans")
    assert items.max() == 120, "inputs: a board with four directions of 30 items fills the table"
    assert_search_equal(host_root(hd, WIDE_FANS[:3], 2, net), sref.search_batch(WIDE_FANS[:3], 2, net), WIDE_FANS[:3], "reference")


@pytest.mark.parametrize("kind", ["mixed", "staged"])
def test_split_mixed_and_staged_networks(hd, kind):
    net = mixed_net() if kind == "mixed" else staged_net()
    boards = near_full_12()
    want2 = reference_search(boards, 2, net)
    assert_search_equal(host_root(hd, boards, 2, net), want2, boards, f"{kind}, root depth 2")
    assert_split_equals_root(hd, boards, 2, net, kind)
    few = boards[:4]
    want3 = reference_search(few, 3, net)
    assert_search_equal(host_root(hd, few, 3, net), want3, few, f"{kind}, root depth 3")
    assert_split_equals_root(hd, boards, 3, net, kind)


@pytest.mark.parametrize("sign", [1, -1])
def test_value_extremes(hd, sign):
    """Weights at +-(2^31 - 1) and F = 16, through ntuple_search_root<3> and the kernel's split.  With the 2^16 / 2^17 tiles
    the issue names, a gain is at most (2^17 + 2^18) << 16 < 2^35 and a chance sum stays near 2^40: those tiles cannot come
    near the int64 bound, so the case that probes it is HUGE.  There a move gains up to 2^30 + 2^29, a value carries three or
    four such gains << 16, about 2^48, and a root chance sum is 10 E = 10..30 times that: the reference reaches 2^52.6 to
    2^53.4 in every direction (asserted: above 2^52 in all, above 2^53 in one), five bits under the 2^58 that the header's
    bound allows.  The issue's 2^55 was not reached: among 6 000 random full boards of such tiles whose reference is
    affordable (at most three empty cells below the root) the largest sum was 2^53.5.  One table of one 4-tuple: |V| = 2^34."""
    dense = random_net(TUPLES_8x4[:1], 0, frac_bits=16)
    dense.weights[:] = sign * ((1 << 31) - 1)
    for board, depth, floor in ((MERGING, 2, 1 << 36), (MERGING, 3, 1 << 36), (HUGE, 3, 1 << 52)):
        sums = chance_sums(board[0], depth, dense)
        mags = [abs(s) for _, _, s in sums.values()]
        assert all(g < 1 << 31 for g, _, _ in sums.values()) and max(mags) > floor
        if board is HUGE:
            assert len(sums) == 4 and min(mags) > 1 << 52 and max(mags) > 1 << 53 and max(mags) < 1 << 58
        want = values_of(sums, 16)
        legal = [d for d in range(4) if d in sums]
        want = (np.array([max(legal, key=lambda d: (int(want[0, d]), -d))], np.uint8), want)
        assert_search_equal(host_root(hd, board, depth, dense), want, board, f"extremes, depth {depth}")
        for P in LANES:
            assert_search_equal(host_split(hd, board, depth, dense, P)[0], want, board, f"extremes, depth {depth}, {P} lanes")
    assert ref.move(ref.plain(MERGING[0]), 3)[1] == 1 << 17 and ref.move(ref.move(ref.plain(MERGING[0]), 3)[0], 3)[1] == 1 << 18


def test_masked_board_is_a_dead_board(hd):
    net = random_net(TUPLES_8x4[:1], 36)
    boards = mixed_boards(6, 37)
    want = host_root(hd, boards, 2, net)
    mask = np.array([1, 0, 7, 0, 0, 1], np.uint32)
    for P in LANES:
        (act, val), items, units = host_split(hd, boards, 2, net, P, active=mask)
        on = mask != 0
        assert np.array_equal(act[on], want[0][on]) and np.array_equal(val[on], want[1][on])
        assert (act[~on] == 0).all() and (val[~on] == sref.ILLEGAL).all() and (items[~on] == 0).all() and (units[~on] == 0).all()


def test_the_table_fits_a_workgroup_s_lds(hd):
    """The kernel's static LDS: the table plus the four wave tables (2 KB) stay far below the 64 KB a workgroup may hold."""
    assert hd.deep_check_lds_bytes() + 2048 < 20 * 1024


def test_arguments_out_of_range_are_refused(hd):
    z = np.zeros(64, np.int64)
    p = z.ctypes.data
    for depth, T, L, F in ((0, 4, 4, 10), (4, 4, 4, 10), (2, 0, 4, 10), (2, 9, 4, 10), (2, 4, 7, 10), (2, 4, 4, 17)):
        assert hd.deep_check_root(p, 1, depth, raw_desc(T, L, F), p, p, p) == -1
    for depth, P in ((1, 64), (4, 64), (2, 0)):
        assert hd.deep_check_split(p, 1, depth, raw_desc(4, 4), p, P, None, p, p, None, None) == -1
