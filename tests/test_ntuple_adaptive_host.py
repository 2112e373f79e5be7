"""CPU: the n-tuple adaptive search of g2048_device.h -- the header the kernels are compiled from -- built for the host
(tests/host_ntuple_adaptive/adaptive_check.cpp, g++).  The split of ntuple_adaptive_search_kernel (the depth of a board from its
empty cells, then root, [leaves1 | expand, scan, leaves, fold], finish over the table the kernel keeps in LDS) run by P simulated
lanes against the header's one-thread root at every depth 0..4; depth 4 against the pure-Python reference on three crafted boards
and against the definition composed from depth-3 roots; a mixed schedule with a mask against the constant-depth results."""
import numpy as np
import pytest

import ntuple_ref as ref
import ntuple_search_ref as sref
from analysis_helpers import ONE_LEGAL, TERMINAL, mixed_boards
from ntuple_adaptive_helpers import (CRAFTED, ILLEGAL, MIXED_SCHEDULE, SKIPPED, compose_next, constant, crafted_net, crafted_reference,
                                     empties_boards, host_root, host_split, load_host_adaptive, named_boards, rows_at)
from ntuple_deep_helpers import (HUGE, LOW_STAGE, SYMMETRIC, anchored_search, extreme_net, implied_root_sums, mixed_net, raw_desc,
                                 reference_rows, reference_search, staged_net)
from ntuple_search_helpers import PAIR_ONLY, WIDE_FANS, assert_search_equal

LANES = (1, 3, 64, 256)
NETS = {"uniform": crafted_net, "staged": staged_net, "mixed": mixed_net}


@pytest.fixture(scope="module")
def ha():
    return load_host_adaptive()


def boards_for(depth):
    """Late boards at every depth; wide and random boards where a one-thread root affords them."""
    if depth == 4:      # (named_boards() at depth 4: test_depth_4_equals_the_composition_of_depth_3_roots)
        return np.concatenate([CRAFTED, LOW_STAGE, PAIR_ONLY, TERMINAL])
    late = np.concatenate([named_boards(), CRAFTED, LOW_STAGE])
    if depth == 3:
        return late
    return np.concatenate([late, WIDE_FANS, mixed_boards(24, 51)])


@pytest.mark.parametrize("kind", list(NETS))
@pytest.mark.parametrize("depth", range(5))
def test_split_equals_the_one_thread_root(ha, depth, kind):
    net, boards = NETS[kind](), boards_for(depth)
    want = host_root(ha, boards, depth, net)
    legal = want[1] != ILLEGAL
    assert legal.any() and (~legal).all(1).any(), "inputs: live boards and a board with no legal move"
    assert (np.abs(want[1][legal]) < 1 << 50).all()
    for P in LANES:
        act, val, dep = host_split(ha, boards, constant(depth), net, P)
        assert_search_equal((act, val), want, boards, f"{kind}, depth {depth}, {P} lanes")
        assert (dep == depth).all()


@pytest.mark.parametrize("depth", [0, 1, 2, 3])
def test_the_one_thread_root_equals_the_reference(ha, depth):
    """Depths 0..3 of the root the other tests compare with, against tests/ntuple_search_ref.py (depth 0: evaluate's q)."""
    net = crafted_net()
    boards = np.concatenate([CRAFTED, PAIR_ONLY, TERMINAL, ONE_LEGAL])
    if depth == 0:
        q, action = ref.evaluate_batch(boards, net)[:2]
        want = (action, q)
    else:
        want = sref.search_batch(boards, depth, net)
    assert_search_equal(host_root(ha, boards, depth, net), want, boards, f"depth {depth}")


def test_depth_4_equals_the_reference(ha):
    """(a) tests/ntuple_search_ref.py at depth 4 on the three crafted boards."""
    want = crafted_reference()
    legal = want[1] != ILLEGAL
    assert legal.sum(1).tolist() == [2, 2, 3], "inputs: the crafted boards have 2, 2 and 3 legal moves"
    assert_search_equal(host_root(ha, CRAFTED, 4, crafted_net()), want, CRAFTED, "root")
    for P in LANES:
        act, val, dep = host_split(ha, CRAFTED, constant(4), crafted_net(), P)
        assert_search_equal((act, val), want, CRAFTED, f"split, {P} lanes")
        assert (dep == 4).all()


@pytest.mark.parametrize("kind", list(NETS))
def test_depth_4_equals_the_composition_of_depth_3_roots(ha, kind):
    """(b) value[d] = (g << F) + (sum of w * S_3(child)) // (10 E), S_3 from the host build's depth-3 root, the top chance level
    in Python integers."""
    net, boards = NETS[kind](), named_boards()
    assert len(boards) == 9
    want, widest, dead = compose_next(boards, net.frac_bits, lambda kids: host_root(ha, kids, 3, net)[1])
    legal = want[1] != ILLEGAL
    assert widest >= 4 and dead >= 1 and legal[:8].any(1).all() and not legal[8].any(), "inputs: a dead child, a dead board"
    assert_search_equal(host_root(ha, boards, 4, net), want, boards, f"{kind}, root")
    for P in LANES:
        act, val, _ = host_split(ha, boards, constant(4), net, P)
        assert_search_equal((act, val), want, boards, f"{kind}, split, {P} lanes")


def test_depth_3_is_composed_the_same_way(ha):
    """The composition itself, one level down, against the reference: depth 3 of near_full(2) from depth-2 roots."""
    from ntuple_deep_helpers import near_full
    boards, net, want3, _, _ = near_full(2)
    got, _, _ = compose_next(boards, net.frac_bits, lambda kids: host_root(ha, kids, 2, net)[1])
    assert_search_equal(got, want3, boards, "composition, depth 3")


@pytest.mark.parametrize("kind", ["max", "random", "min"])
def test_value_extremes_depth_4(ha, kind):
    """Depth 4 at the header's bounds on the CPU: one 4-tuple with every weight INT32_MAX, every weight INT32_MIN or one of the two
    at random, F = 16, the networks and the expected values of tests/test_gpu_ntuple_deep_extremes.py.  SYMMETRIC (tiles of 2^27 ..
    2^29, one empty cell, equal to its transpose) goes straight against tests/ntuple_search_ref.py: values of 2^48, a root tie.
    HUGE, whose depth-4 reference would take minutes, is composed under the random fill: the top chance sum and its floor
    division in Python integers over the host build's depth-3 values of the children, a quarter of which are composed the same way
    from depth-2 values, a quarter of which equal the reference (anchored_search).  Its root chance sums pass 2^52."""
    net = extreme_net(kind, 16, 1)
    want = reference_rows(SYMMETRIC, 4, net)
    sums = implied_root_sums(SYMMETRIC, want[1], 16)[0]
    legal = want[1][0] != ILLEGAL
    assert legal.all() and min(sums) > 1 << 50 and (want[1] > 1 << 47).all() and (np.abs(want[1]) < 1 << 50).all()
    assert want[1][0, 0] == want[1][0, 3] and want[1][0, 1] == want[1][0, 2] and want[0][0] == want[1][0].argmax(), "inputs: a root tie"
    cases = [(SYMMETRIC, want)]
    if kind == "random":
        stats = {}
        composed = anchored_search(HUGE, 4, net, lambda kids, k: host_root(ha, kids, k, net), lambda board: 2, stats)
        top = implied_root_sums(HUGE, composed[1], 16)[0]
        assert stats["composed"] >= 9 and 4 * stats["anchored"] >= stats["children"] and stats["direct"] >= 64
        assert len(top) == 4 and max(top) > 1 << 52 and max(top) < 1 << 58
        cases.append((HUGE, composed))
    for board, expect in cases:
        assert_search_equal(host_root(ha, board, 4, net), expect, board, f"{kind}, root")
        for P in LANES if board is SYMMETRIC else LANES[-1:]:      # (HUGE at depth 4 takes the host build 2.5 s a run)
            act, val, dep = host_split(ha, board, constant(4), net, P)
            assert_search_equal((act, val), expect, board, f"{kind}, split, {P} lanes")
            assert (dep == 4).all()


LEAN_SCHEDULE = tuple(min(d, 3) for d in MIXED_SCHEDULE)        # the same rule cut at depth 3


@pytest.mark.parametrize("kind", list(NETS))
@pytest.mark.parametrize("schedule", [MIXED_SCHEDULE, LEAN_SCHEDULE], ids=["to depth 4", "to depth 3"])
def test_a_mixed_schedule_with_a_mask(ha, schedule, kind):
    """17 boards with 0..16 empty cells under a schedule that uses every depth: each board equals its own constant-depth root,
    depth = schedule[E0]; with every other board masked out, those are dead with depth 0xff and the others unchanged."""
    net, boards = NETS[kind](), empties_boards()
    rows, depths = rows_at(schedule, boards)
    assert sorted(rows) == list(range(max(schedule) + 1)) and depths.tolist() == list(schedule)
    want = (np.zeros(17, np.uint8), np.zeros((17, 4), np.int64))
    for depth, at in rows.items():
        a, v = host_root(ha, boards[at], depth, net)
        want[0][at], want[1][at] = a, v
    assert (want[1][:16] != ILLEGAL).any(1).all() and (want[1][16] == ILLEGAL).all(), "inputs: only the empty board is dead"
    mask = np.where(np.arange(17) % 2 == 0, 0, [1, 7, 1 << 31, 0xffffffff] * 4 + [1]).astype(np.uint32)
    for P in LANES:
        act, val, dep = host_split(ha, boards, schedule, net, P)
        assert_search_equal((act, val), want, boards, f"{kind}, {P} lanes")
        assert dep.tolist() == list(schedule)
        act, val, dep = host_split(ha, boards, schedule, net, P, active=mask)
        on = mask != 0
        assert_search_equal((act[on], val[on]), (want[0][on], want[1][on]), boards[on], f"{kind}, masked, {P} lanes")
        assert (act[~on] == 0).all() and (val[~on] == ILLEGAL).all() and (dep[~on] == SKIPPED).all()
        assert dep[on].tolist() == depths[on].tolist()


def test_the_order_of_boards_does_not_matter(ha):
    """The table is reused from board to board: a cheap board after a depth-4 board and the reverse give the same bits."""
    net, boards = crafted_net(), empties_boards()
    fwd = host_split(ha, boards, MIXED_SCHEDULE, net, 64)
    rev = host_split(ha, boards[::-1], MIXED_SCHEDULE, net, 64)
    for f, r in zip(fwd, rev):
        assert np.array_equal(f, r[::-1])


def test_staged_depth_3_equals_the_reference(ha):
    net = staged_net()
    few = named_boards()[:3]
    act, val, _ = host_split(ha, few, constant(3), net, 256)
    assert_search_equal((act, val), reference_search(few, 3, net), few, "staged, depth 3")


def test_arguments_out_of_range_are_refused(ha):
    z = np.zeros(64, np.int64)
    p = z.ctypes.data
    sched = np.zeros(17, np.uint8)
    for depth, T, L, F in ((5, 4, 4, 10), (2, 0, 4, 10), (2, 9, 4, 10), (2, 4, 7, 10), (2, 4, 4, 17)):
        assert ha.adaptive_check_root(p, 1, depth, raw_desc(T, L, F), p, p, p) == -1
    assert ha.adaptive_check_split(p, 1, sched.ctypes.data, raw_desc(4, 4), p, 0, None, p, p, p) == -1
    assert ha.adaptive_check_split(p, 1, None, raw_desc(4, 4), p, 64, None, p, p, p) == -1
    for e in (0, 9, 16):
        bad = sched.copy()
        bad[e] = 5
        assert ha.adaptive_check_split(p, 1, bad.ctypes.data, raw_desc(4, 4), p, 64, None, p, p, p) == -1
