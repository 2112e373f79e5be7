"""CPU: the n-tuple expectimax of g2048_device.h -- the header the kernels are compiled from -- built for the host
(tests/host_ntuple/ntuple_check.cpp, g++) and compared bit for bit with the pure-Python reference
tests/ntuple_search_ref.py.  Every named case shows from the reference's own trace (never from the code under test) that
its input reaches the edge it names."""
import numpy as np
import pytest

import ntuple_ref as ref
import ntuple_search_ref as sref
from analysis_helpers import ONE_LEGAL, TERMINAL, mid_game, mixed_boards, random_boards
from ntuple_helpers import (TUPLES_2x6, TUPLES_8x4, TUPLES_8x6, TUPLES_17x4, host_search, host_split, load_host_ntuple, random_net,
                            raw_desc)
from ntuple_search_helpers import PAIR_ONLY, WIDE_FANS, assert_search_equal

@pytest.fixture(scope="module")
def hs():
    return load_host_ntuple()


def check(lib, boards, depth, net):
    """host == reference; returns (the reference's (action, value), its trace)."""
    trace = sref.Trace()
    want = sref.search_batch(boards, depth, net, trace)
    assert_search_equal(host_search(lib, boards, depth, net), want, boards, f"depth {depth}")
    return want, trace


def test_floor_div(hs):
    """The one named helper: floors where C++ truncates."""
    for a, b in ((-7, 10), (-10, 10), (-11, 10), (7, 10), (0, 150), (-1, 150), (-(1 << 57) - 1, 150), ((1 << 57) + 1, 150), (-149, 150)):
        assert hs.ntuple_check_floor_div(a, b) == a // b, (a, b)


@pytest.mark.parametrize("tuples", [TUPLES_17x4, TUPLES_2x6], ids=["17x4", "2x6"])
def test_depth_1_mixed_boards(hs, tuples):
    net = random_net(tuples, 21)
    boards = np.concatenate([mixed_boards(300, 21), ONE_LEGAL, TERMINAL])
    (act, val), trace = check(hs, boards, 1, net)
    legal = val != sref.ILLEGAL
    assert trace.chance > 800 and trace.negative_inexact > 100 and (~legal).any() and len(set(act.tolist())) == 4
    assert (val[legal] < 0).any() and (val[legal] > 0).any()
    # look-ahead is not the greedy player: the depth-1 action differs from evaluate's on some boards
    assert (act != ref.greedy_actions(boards, net)).any()


def test_depth_2_near_full_boards(hs):
    net = random_net(TUPLES_17x4, 22)
    boards = np.concatenate([mid_game(30, 22, max_empty=3), PAIR_ONLY])
    assert ((boards == 0).sum(1) <= 3).all()
    _, trace = check(hs, boards, 2, net)
    assert trace.chance > 1000 and trace.negative_inexact > 100 and trace.terminal_children > 0


@pytest.mark.parametrize("depth, boards, tuples", [(1, mixed_boards(60, 23), TUPLES_17x4), (2, mid_game(8, 23, max_empty=3), TUPLES_17x4),
                                                   (2, WIDE_FANS, TUPLES_8x4[:1])], ids=["depth1", "depth2", "depth2-wide"])
def test_lane_split_sums_to_the_one_thread_sum(hs, depth, boards, tuples):
    """The kernel's split: the parts of K lanes add up to the whole chance sum, for K lanes per direction in {1, 4, 16}.
    The wide boards give a direction up to 30 items: with K = 16 lanes take a second item, with K = 4 up to eight (the
    one-tuple network keeps the reference at about 9 s)."""
    net = random_net(tuples, 23)
    whole = host_split(hs, boards, depth, net, 1)
    trace = sref.Trace()
    _, val = sref.search_batch(boards, depth, net, trace)
    legal = val != sref.ILLEGAL
    if boards is WIDE_FANS:
        assert max(trace.root_items) == 30 and {16, 18, 24, 30} <= set(trace.root_items)
    else:
        assert depth == 1 or max(trace.root_items) < 16      # (the near-full boards never give a lane a second item)
    # the whole sum is the reference's: floor(sum / 10E) + (gain << F) = value
    for i, b in enumerate(boards):
        for d in range(4):
            a, g, ok = ref.move(ref.plain(b), d)
            if ok:
                assert int(whole[i, d]) // (10 * sum(x == 0 for x in a)) + (g << net.frac_bits) == val[i, d]
    assert (whole[~legal] == 0).all() and (whole[legal] != 0).any()
    for K in (4, 16):
        assert np.array_equal(host_split(hs, boards, depth, net, K), whole), K


def test_negative_inexact_chance_sums(hs):
    """All-negative weights: a chance sum is negative (or 0, when every child is terminal), and those not divisible by 10E
    must floor, not truncate."""
    net = random_net(TUPLES_17x4, 24, lo=-(1 << 31), hi=-(1 << 29))
    boards = np.concatenate([random_boards(40, 25), ONE_LEGAL])
    (act, val), trace = check(hs, boards, 1, net)
    legal = val != sref.ILLEGAL
    assert trace.negative_inexact > 0.8 * trace.chance > 50 and (val[legal] < 0).sum() > 100
    assert legal[np.arange(len(act)), act][legal.any(1)].all() and act[-1] == 2   # the action is a legal move although every value < 0


def test_terminal_child(hs):
    """A chance child with no legal move counts S = 0."""
    net = random_net(TUPLES_17x4, 26)
    want = {}
    for d in (1, 3):
        after, g, legal = ref.move(ref.plain(PAIR_ONLY[0]), d)
        (c,) = [c for c in range(16) if after[c] == 0]
        dead, alive = after[:c] + (1,) + after[c + 1:], after[:c] + (2,) + after[c + 1:]
        assert legal and g == 4 and not any(ref.move(dead, m)[2] for m in range(4)) and any(ref.move(alive, m)[2] for m in range(4))
        want[d] = (4 << net.frac_bits) + (9 * 0 + sref.state_value(alive, 0, net)) // 10
    assert not ref.move(ref.plain(PAIR_ONLY[0]), 0)[2] and not ref.move(ref.plain(PAIR_ONLY[0]), 2)[2]
    (act, val), trace = check(hs, PAIR_ONLY, 1, net)
    assert trace.terminal_children == 2 and trace.chance == 2
    assert val[0].tolist() == [sref.ILLEGAL, want[1], sref.ILLEGAL, want[3]] and act[0] == (1 if want[1] >= want[3] else 3)
    _, trace2 = check(hs, PAIR_ONLY, 2, net)
    assert trace2.terminal_children >= 2


def test_root_tie_takes_the_smallest_direction(hs):
    net = ref.Net(TUPLES_17x4, 10)                                      # zero weights: a value is expected merge scores only
    lone = np.array([[0] * 5 + [3] + [0] * 10], np.uint8)               # no merge within two moves whatever is done
    pair = np.array([[1, 1] + [0] * 14], np.uint8)                      # up illegal; right and left are mirror images
    (act, val), trace = check(hs, np.concatenate([lone, pair]), 1, net)
    assert trace.root_ties == 2
    assert val[0].tolist() == [0, 0, 0, 0] and act[0] == 0
    assert val[1, 0] == sref.ILLEGAL and val[1, 1] == val[1, 3] > val[1, 2] and act[1] == 1


def test_one_legal_and_terminal(hs):
    net = random_net(TUPLES_2x6, 27)
    for depth in (1, 2):
        (act, val), _ = check(hs, np.concatenate([ONE_LEGAL, TERMINAL]), depth, net)
        assert act[0] == 2 and (val[0, [0, 1, 3]] == sref.ILLEGAL).all() and val[0, 2] != sref.ILLEGAL
        assert act[1] == 0 and (val[1] == sref.ILLEGAL).all()


def test_exponents_at_and_past_the_clamp(hs):
    """Exponents 15, 16, 17 and 31 share the last table row; the boards keep their own exponents for the moves (a 31
    merges with a 31, not with a 15)."""
    net = random_net(TUPLES_17x4, 28)
    base = random_boards(10, 29, max_exp=12)
    boards = []
    for b in base:
        for e in (14, 15, 16, 17, 31):
            x = b.copy()
            x[[0, 1, 10, 15]] = [e, e, 15, 2]
            boards.append(x)
    boards = np.array(boards, np.uint8)
    (_, val), _ = check(hs, boards, 1, net)
    merged = [ref.move(ref.plain(b), 3) for b in boards[4::5]]           # left merges the two 31s into a 32: gain 2^(32 mod 32)
    assert all(a[0] == 32 and g >= 1 for a, g, _ in merged)
    full = np.array([[31, 31, 17, 16, 15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 0, 5]], np.uint8)
    check(hs, full, 2, net)                                              # depth 2 through 31 + 31 -> 32


@pytest.mark.parametrize("tuples", [((9,),), TUPLES_8x6], ids=["T1L1", "T8L6"])
def test_smallest_and_largest_shape(hs, tuples):
    net = random_net(tuples, 30)
    (_, val), trace = check(hs, np.concatenate([random_boards(20, 31), np.array([[15, 16, 17, 31] * 3 + [0, 0, 15, 31]], np.uint8)]), 1, net)
    assert trace.chance > 40 and (val != sref.ILLEGAL).any()
    check(hs, mid_game(3, 31, max_empty=2), 2, net)


@pytest.mark.parametrize("frac_bits", [0, 16])
def test_frac_bits_at_both_ends(hs, frac_bits):
    """F = 0: a gain counts as itself; F = 16: a gain of 2^17 adds 2^33 to a value.  The gains must show in the values."""
    net = random_net(TUPLES_17x4, 32, frac_bits=frac_bits, lo=-1000, hi=1000)
    boards = np.concatenate([random_boards(30, 33), np.array([[16, 16, 3, 0, 0, 2, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0]], np.uint8)])
    (_, val), _ = check(hs, boards, 1, net)
    assert ref.move(ref.plain(boards[-1]), 3)[1] == 1 << 17 and val[-1, 3] > (1 << 16) << frac_bits   # |V| <= 40 000 < 2^16
    check(hs, mid_game(4, 33, max_empty=2), 2, net)


def test_arguments_out_of_range_are_refused(hs):
    z = np.zeros(64, np.int64)
    p = z.ctypes.data
    for depth, T, L, F in ((0, 4, 4, 10), (3, 4, 4, 10), (1, 0, 4, 10), (1, 9, 4, 10), (1, 4, 7, 10), (1, 4, 4, 17)):
        assert hs.ntuple_check_search(p, 1, depth, raw_desc(T, L, F), p, p, p) == -1
