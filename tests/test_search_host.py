"""CPU: the expectimax code of g2048_device.h -- the header the search kernels are compiled from -- built for the host
(tests/host_check/host_check.cpp, g++) and compared bit for bit with the pure-Python reference tests/search_ref.py."""
import numpy as np
import pytest

import search_ref as ref
from analysis_helpers import (I32x4, afterstate_empties, high_boards, host_search, host_split, hs,  # noqa: F401 (hs: fixture)
                              random_boards, trajectory_boards)


def check(lib, boards, depth, w=ref.DEFAULT_WEIGHTS):
    act, val = host_search(lib, boards, depth, w)
    ract, rval = ref.search_batch(boards, depth, w)
    bad = np.nonzero((act != ract) | (val != rval).any(1))[0]
    assert len(bad) == 0, f"{len(bad)} boards differ, first {boards[bad[0]].tolist()}: {act[bad[0]]} {val[bad[0]]} " \
                          f"vs {ract[bad[0]]} {rval[bad[0]]}"
    return act, val


def test_heuristic(hs):
    boards = random_boards(2000, 1, max_exp=31)
    for w in (ref.DEFAULT_WEIGHTS, (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1 << 24, 65535, 65535, 65535)):
        for b in boards:
            assert hs.search_check_heuristic(np.ascontiguousarray(b).ctypes.data, I32x4(*w)) == ref.heuristic(tuple(int(x) for x in b), w)


def test_heuristic_bound():
    """H < 2^27 at the largest weights, on the worst line the exponents allow (34 = 31 + three merges)."""
    worst = (34, 33, 34, 33) * 4
    assert ref.heuristic(worst, (1 << 24, 65535, 65535, 65535)) < 1 << 27
    assert ref.heuristic((0,) * 16, (1 << 24, 65535, 65535, 65535)) < 1 << 27


def test_depth1_random(hs):
    check(hs, random_boards(3000, 2), 1)


def test_depth1_trajectories(hs):
    boards = trajectory_boards(every=7)
    assert len(boards) > 1000
    check(hs, boards, 1)


def test_depth1_weights_and_mod32(hs):
    boards = random_boards(400, 3, max_exp=31)
    check(hs, boards, 1, (1 << 24, 65535, 65535, 65535))
    check(hs, boards, 1, (0, 0, 0, 0))
    check(hs, boards, 1, (7, 3, 65535, 1))
    # the plain form takes exponents mod 32 (g2048_afterstates_plain)
    hi = boards | np.where(boards > 0, 32, 0).astype(np.uint8)
    assert all(np.array_equal(x, y) for x, y in zip(host_search(hs, hi, 1), host_search(hs, boards, 1)))


def test_depth2(hs):
    boards = np.concatenate([random_boards(24, 4), trajectory_boards(every=997)[:16]])
    assert len(boards) >= 32
    check(hs, boards, 2)
    check(hs, boards[:8], 2, (1 << 24, 65535, 65535, 65535))


def test_depth3(hs):
    rng = np.random.default_rng(5)
    boards = random_boards(200, 6)
    boards = boards[(boards == 0).sum(1) <= 6][:4]  # few empty cells keep the Python tree small
    boards = np.concatenate([boards, trajectory_boards(every=1)[rng.integers(0, 1000, 1)]])
    check(hs, boards, 3)


@pytest.mark.parametrize("name", sorted(ref.HAND_CASES))
def test_hand_cases(hs, name):
    board, depth, w, expected = ref.HAND_CASES[name]
    act, val = check(hs, board[None], depth, w)
    if expected is not None:
        assert act[0] == expected
    if name == "dead":
        assert (val[0] == -1).all()
    if name == "one_legal_move":
        assert (val[0] >= 0).sum() == 1
    if name == "tie_right_left":
        assert val[0, 1] == val[0, 3] >= 0 and val[0, 0] == val[0, 2] == -1
    if name == "empty_from_merge":
        assert (board == 0).sum() == 0 and (val[0] >= 0).any()
    if name == "zero_weights":
        assert (val[0][val[0] >= 0] == 0).all()
    for d in range(1, 4) if name != "max_weights" else (1,):
        check(hs, board[None], d, w)


@pytest.mark.parametrize("depth,K", [(1, 4), (1, 16), (2, 16), (2, 3), (3, 16)])
def test_lane_split(hs, depth, K):
    """The kernels' split (K lanes per direction, partial sums added before the one divide) gives the same values."""
    boards = random_boards({1: 500, 2: 40, 3: 3}[depth], 7)
    if depth == 3:
        boards = boards[(boards == 0).sum(1) <= 6][:2]
    _, val = host_search(hs, boards, depth)
    assert np.array_equal(host_split(hs, boards, depth, K), val)


@pytest.mark.parametrize("w", [ref.DEFAULT_WEIGHTS, ref.MAX_WEIGHTS], ids=["default", "max"])
def test_near_top_exponents_depth2_depth3(hs, w):
    """Exponents 26..31 with equal neighbours: the merges inside the tree make exponents 32..34, which the byte tricks of
    line_terms / shift4 must carry (the header's claim).  Depth 2 on 12 boards, depth 3 on 3 (few empty cells)."""
    b2 = np.concatenate([high_boards(6, 40, (1, 5)), high_boards(6, 42, (1, 4), full_rows=1)])
    b3 = high_boards(2, 41, (1, 3), full_rows=2)
    check(hs, b2, 2, w)
    check(hs, b3, 3, w)
    # the inputs reach the edge: every tree goes past 31, the depth-2 trees to 33, the depth-3 trees to 34
    tops2, tops3 = [ref.max_exponent(b, 2) for b in b2], [ref.max_exponent(b, 3) for b in b3]
    assert min(tops2) >= 32 and max(tops2) == 33 and tops3 == [34] * len(b3), (tops2, tops3)


@pytest.mark.parametrize("depth,n", [(2, 40), (3, 3)])
def test_lane_split_wide_sums(hs, depth, n):
    """The kernels' split at K = 16 with the largest weights, where a root's chance sum is wider than 32 bits: the
    64-bit partial sums of 16 lanes must add up to the one-lane sum."""
    boards = high_boards(n, 50 + depth, (6, 10))
    _, val = host_search(hs, boards, depth, ref.MAX_WEIGHTS)
    assert np.array_equal(host_split(hs, boards, depth, 16, ref.MAX_WEIGHTS), val)
    E = afterstate_empties(boards)
    # value = floor(total / 10E), so value * 10E <= total: these roots summed past 2^32
    wide = (val >= 0) & (val.astype(np.int64) * 10 * E >= 1 << 32)
    assert wide.sum() * 4 >= (val >= 0).sum(), (wide.sum(), (val >= 0).sum())
    if depth == 2:  # the undivided sums themselves, from the Python reference
        totals = [ref.root_totals(b, 2, ref.MAX_WEIGHTS) for b in boards[:6]]
        assert max(t for row in totals for t in row if t is not None) >= 1 << 32
        for row, v, e in zip(totals, val, E):
            assert [-1 if t is None else t // (10 * k) for t, k in zip(row, e)] == v.tolist()
