"""CPU: the n-tuple reduced search of g2048_device.h -- the header the kernels are compiled from -- built for the host
(tests/host_ntuple_reduced/reduced_check.cpp, g++).  The split of ntuple_reduced_search_kernel (root, [leaves1 | expand, scan,
leaves, fold], finish over the table the kernel keeps in LDS) run by P simulated lanes against the one-thread recursion of the
definition at every depth 0..4 and both reductions; that recursion against the pure-Python reference
(tests/ntuple_reduced_ref.py); the identities at depth 0 and 1 and the composition of one chance level with two child depths; a
mixed schedule with a mask; the value extremes at depth 4."""
import numpy as np
import pytest

import ntuple_reduced_ref as rref
import ntuple_ref as ref
import ntuple_search_ref as sref
from ntuple_adaptive_helpers import (CRAFTED, ILLEGAL, MIXED_SCHEDULE, SKIPPED, constant, crafted_net, empties_boards, named_boards,
                                     rows_at)
from ntuple_adaptive_helpers import host_root as adaptive_root, load_host_adaptive
from ntuple_deep_helpers import HUGE, SYMMETRIC, extreme_net, implied_root_sums, mixed_net, raw_desc, staged_net
from ntuple_reduced_helpers import (REDUCE4, STATE_BOARDS, TIED, boards_for, compose_reduced, evaluations, host_root, host_split,
                                    host_unit, load_host_reduced)
from ntuple_search_helpers import assert_search_equal

LANES = (1, 3, 64, 256)
NETS = {"uniform": crafted_net, "staged": staged_net, "mixed": mixed_net}


@pytest.fixture(scope="module")
def hr():
    return load_host_reduced()


@pytest.fixture(scope="module")
def ha():
    return load_host_adaptive()


@pytest.mark.parametrize("kind", list(NETS))
@pytest.mark.parametrize("R", REDUCE4)
@pytest.mark.parametrize("depth", range(5))
def test_split_equals_the_one_thread_root(hr, depth, R, kind):
    net, boards = NETS[kind](), boards_for(depth)
    want = host_root(hr, boards, depth, R, net)
    legal = want[1] != ILLEGAL
    assert legal.any() and (~legal).all(1).any(), "inputs: live boards and a board with no legal move"
    assert (np.abs(want[1][legal]) < 1 << 50).all()
    for P in LANES:
        act, val, dep = host_split(hr, boards, constant(depth), R, net, P)
        assert_search_equal((act, val), want, boards, f"{kind}, depth {depth}, R {R}, {P} lanes")
        assert (dep == depth).all(), "the depth output is the schedule's depth, not a reduced one"


@pytest.mark.parametrize("R", REDUCE4)
@pytest.mark.parametrize("depth", [0, 1, 2, 3])
def test_the_one_thread_root_equals_the_reference(hr, depth, R):
    """Depths 0..3 of the root the other tests compare with, against tests/ntuple_reduced_ref.py, on boards that reach every new
    state of the table: shown from the reference's own trace."""
    net, trace = crafted_net(), rref.Trace()
    want = rref.search_batch(STATE_BOARDS, depth, R, net, trace)
    if depth >= 1:
        assert trace.root_ties >= 1, "inputs: a root tie"
    if depth >= 2:
        assert trace.terminal_level1 >= 1, "inputs: a level-1 child with no legal move"
        assert trace.negative_inexact >= 1, "inputs: a negative chance sum with an inexact quotient"
    if depth == 2 or (depth == 3 and R == 2):
        assert trace.leaf_beside_units >= 1, "inputs: a legal 4 child that is a leaf entry while its 2 sibling has units"
        assert set(trace.level1_depths) == {0, depth - 1}
    if depth == 3 and R == 1:
        assert set(trace.level1_depths) == {1, 2}
    assert_search_equal(host_root(hr, STATE_BOARDS, depth, R, net), want, STATE_BOARDS, f"depth {depth}, R {R}")
    for P in LANES:
        act, val, _ = host_split(hr, STATE_BOARDS, constant(depth), R, net, P)
        assert_search_equal((act, val), want, STATE_BOARDS, f"split, depth {depth}, R {R}, {P} lanes")


@pytest.mark.parametrize("R", REDUCE4)
def test_depth_4_equals_the_reference(hr, R):
    """tests/ntuple_reduced_ref.py at depth 4 on the three crafted boards and the tied one: half a second a board, where the full
    depth-4 reference takes 0.6 s."""
    net, trace, boards = crafted_net(), rref.Trace(), np.concatenate([CRAFTED, TIED])
    want = rref.search_batch(boards, 4, R, net, trace)
    assert (want[1] != ILLEGAL).sum(1).tolist() == [2, 2, 3, 4], "inputs: the boards have 2, 2, 3 and 4 legal moves"
    assert trace.root_ties >= 1 and trace.negative_inexact >= 1 and trace.terminal_children >= 1
    assert set(trace.level1_depths) == {3, 3 - R}
    if R == 2:
        assert trace.level1_depths[1] >= 1, "inputs: at D = 4, R = 2, an item with r1 = 1"
    assert_search_equal(host_root(hr, boards, 4, R, net), want, boards, f"root, R {R}")
    for P in LANES:
        act, val, dep = host_split(hr, boards, constant(4), R, net, P)
        assert_search_equal((act, val), want, boards, f"split, R {R}, {P} lanes")
        assert (dep == 4).all()


def test_the_reduced_search_costs_less_than_the_full_one():
    """Leaf evaluations counted from the definition: what the reduction is for, and that R = 2 cuts no less than R = 1."""
    for b in CRAFTED:
        full, one, two = (evaluations(b, 4, R) for R in (0, 1, 2))
        assert two <= one < full
    assert evaluations(CRAFTED[0], 1, 0) == evaluations(CRAFTED[0], 1, 2), "depth 1 reduces nothing"


@pytest.mark.parametrize("kind", list(NETS))
@pytest.mark.parametrize("R", REDUCE4)
def test_depth_0_and_1_are_the_adaptive_search(hr, ha, R, kind):
    """D = 0 is evaluate's value and action and D = 1 the depth-1 search, bit for bit, for any R: against the adaptive host
    build's roots (themselves checked against the references in tests/test_ntuple_adaptive_host.py) and, for the uniform
    network, the pure-Python references directly."""
    net, boards = NETS[kind](), np.concatenate([named_boards(), TIED])
    for depth in (0, 1):
        want = adaptive_root(ha, boards, depth, net)
        assert_search_equal(host_root(hr, boards, depth, R, net), want, boards, f"{kind}, root, depth {depth}")
        for P in LANES:
            act, val, _ = host_split(hr, boards, constant(depth), R, net, P)
            assert_search_equal((act, val), want, boards, f"{kind}, split, depth {depth}, {P} lanes")
    if kind == "uniform":
        q, action = ref.evaluate_batch(boards, net)[:2]
        assert_search_equal(host_root(hr, boards, 0, R, net), (action, q), boards, "evaluate")
        assert_search_equal(host_root(hr, boards, 1, R, net), sref.search_batch(boards, 1, net), boards, "search(1)")


@pytest.mark.parametrize("kind", list(NETS))
@pytest.mark.parametrize("R", REDUCE4)
@pytest.mark.parametrize("depth", [2, 3, 4])
def test_one_chance_level_composed_in_python(hr, ha, depth, R, kind):
    """value^R_D(b) = (g << F) + (sum of 9 S^R_{D-1}(2 child) + S^R_{max(D-1-R,0)}(4 child)) // (10 E) in Python integers.  The
    children's values come from this call's split at the lower constant depths, and from the adaptive host build's roots at
    depth <= 1, where the two searches are the same."""
    net, boards = NETS[kind](), named_boards()
    assert len(boards) == 9

    def state_values(kids, k):
        if k <= 1:
            return adaptive_root(ha, kids, k, net)[1]
        return host_split(hr, kids, constant(k), R, net, 64)[1]

    want, dead = compose_reduced(boards, net.frac_bits, depth, R, state_values)
    legal = want[1] != ILLEGAL
    assert dead >= 1 and legal[:8].any(1).all() and not legal[8].any(), "inputs: a dead child, a dead board"
    assert_search_equal(host_root(hr, boards, depth, R, net), want, boards, f"{kind}, root")
    for P in LANES:
        act, val, _ = host_split(hr, boards, constant(depth), R, net, P)
        assert_search_equal((act, val), want, boards, f"{kind}, split, {P} lanes")


@pytest.mark.parametrize("kind", list(NETS))
def test_the_unit_tree_of_a_lane(hr, ha, kind):
    """ntuple_reduced_state, the tree a lane runs for a work unit: S_0 and S_1 are the largest legal value of the depth-0 and
    depth-1 searches, and S^R_2 that of the reduced depth-2 root (the same for both R), 0 for a board with no legal move."""
    net, boards = NETS[kind](), np.concatenate([named_boards(), TIED])

    def best(value):
        return np.array([max(int(x) for x in row[row != ILLEGAL]) if (row != ILLEGAL).any() else 0 for row in value], np.int64)

    assert np.array_equal(host_unit(hr, boards, 0, net), best(adaptive_root(ha, boards, 0, net)[1]))
    assert np.array_equal(host_unit(hr, boards, 1, net), best(adaptive_root(ha, boards, 1, net)[1]))
    two = best(host_root(hr, boards, 2, 1, net)[1])
    assert np.array_equal(two, best(host_root(hr, boards, 2, 2, net)[1]))
    assert np.array_equal(host_unit(hr, boards, 2, net), two)
    assert (two == 0).any() and (two != 0).any()


@pytest.mark.parametrize("kind", list(NETS))
@pytest.mark.parametrize("R", REDUCE4)
def test_a_mixed_schedule_with_a_mask(hr, R, kind):
    """17 boards with 0..16 empty cells under a schedule that uses every depth: each board equals its own constant-depth root,
    depth = schedule[E0]; with every other board masked out, those are dead with depth 0xff and the others unchanged."""
    net, boards, schedule = NETS[kind](), empties_boards(), MIXED_SCHEDULE
    rows, depths = rows_at(schedule, boards)
    assert sorted(rows) == list(range(5)) and depths.tolist() == list(schedule)
    want = (np.zeros(17, np.uint8), np.zeros((17, 4), np.int64))
    for depth, at in rows.items():
        a, v = host_root(hr, boards[at], depth, R, net)
        want[0][at], want[1][at] = a, v
    assert (want[1][:16] != ILLEGAL).any(1).all() and (want[1][16] == ILLEGAL).all(), "inputs: only the empty board is dead"
    mask = np.where(np.arange(17) % 2 == 0, 0, [1, 7, 1 << 31, 0xffffffff] * 4 + [1]).astype(np.uint32)
    for P in LANES:
        act, val, dep = host_split(hr, boards, schedule, R, net, P)
        assert_search_equal((act, val), want, boards, f"{kind}, {P} lanes")
        assert dep.tolist() == list(schedule)
        act, val, dep = host_split(hr, boards, schedule, R, net, P, active=mask)
        on = mask != 0
        assert_search_equal((act[on], val[on]), (want[0][on], want[1][on]), boards[on], f"{kind}, masked, {P} lanes")
        assert (act[~on] == 0).all() and (val[~on] == ILLEGAL).all() and (dep[~on] == SKIPPED).all()
        assert dep[on].tolist() == depths[on].tolist()


def test_the_order_of_boards_does_not_matter(hr):
    """The table is reused from board to board: a cheap board after a depth-4 board and the reverse give the same bits."""
    net, boards = crafted_net(), empties_boards()
    fwd = host_split(hr, boards, MIXED_SCHEDULE, 1, net, 64)
    rev = host_split(hr, boards[::-1], MIXED_SCHEDULE, 1, net, 64)
    for f, r in zip(fwd, rev):
        assert np.array_equal(f, r[::-1])


@pytest.mark.parametrize("kind", ["max", "random", "min"])
def test_value_extremes_depth_4(hr, kind):
    """Depth 4, R = 1 at the header's bounds: the boards and networks of test_value_extremes_depth_4 of
    tests/test_ntuple_adaptive_host.py.  SYMMETRIC (tiles of 2^27 .. 2^29, one empty cell, equal to its transpose) goes straight
    against tests/ntuple_reduced_ref.py: values of 2^48, a root tie.  HUGE is composed under the random fill: the top chance
    level in Python integers over the split's depth-3 and depth-2 values of the children.  Its root chance sums pass 2^52."""
    net = extreme_net(kind, 16, 1)
    want = rref.search_batch(SYMMETRIC, 4, 1, net)
    sums = implied_root_sums(SYMMETRIC, want[1], 16)[0]
    legal = want[1][0] != ILLEGAL
    assert legal.all() and min(sums) > 1 << 50 and (want[1] > 1 << 47).all() and (np.abs(want[1]) < 1 << 50).all()
    assert want[1][0, 0] == want[1][0, 3] and want[1][0, 1] == want[1][0, 2] and want[0][0] == want[1][0].argmax(), "inputs: a root tie"
    cases = [(SYMMETRIC, want)]
    if kind == "random":
        composed, _ = compose_reduced(HUGE, 16, 4, 1, lambda kids, k: host_split(hr, kids, constant(k), 1, net, 64)[1])
        top = implied_root_sums(HUGE, composed[1], 16)[0]
        assert len(top) == 4 and max(top) > 1 << 52 and max(top) < 1 << 58
        cases.append((HUGE, composed))
    for board, expect in cases:
        assert_search_equal(host_root(hr, board, 4, 1, net), expect, board, f"{kind}, root")
        for P in LANES if board is SYMMETRIC else LANES[-1:]:
            act, val, dep = host_split(hr, board, constant(4), 1, net, P)
            assert_search_equal((act, val), expect, board, f"{kind}, split, {P} lanes")
            assert (dep == 4).all()


def test_arguments_out_of_range_are_refused(hr):
    z = np.zeros(64, np.int64)
    p = z.ctypes.data
    sched = np.zeros(17, np.uint8)
    for depth, R, T, L, F in ((5, 1, 4, 4, 10), (2, 0, 4, 4, 10), (2, 3, 4, 4, 10), (2, 1, 0, 4, 10), (2, 1, 9, 4, 10), (2, 1, 4, 7, 10),
                              (2, 1, 4, 4, 17)):
        assert hr.reduced_check_root(p, 1, depth, R, raw_desc(T, L, F), p, p, p) == -1
    assert hr.reduced_check_unit(p, 1, 3, raw_desc(4, 4), p, p) == -1
    assert hr.reduced_check_split(p, 1, sched.ctypes.data, 1, raw_desc(4, 4), p, 0, None, p, p, p) == -1
    assert hr.reduced_check_split(p, 1, None, 1, raw_desc(4, 4), p, 64, None, p, p, p) == -1
    for R in (0, 3):
        assert hr.reduced_check_split(p, 1, sched.ctypes.data, R, raw_desc(4, 4), p, 64, None, p, p, p) == -1
    bad = sched.copy()
    bad[9] = 5
    assert hr.reduced_check_split(p, 1, bad.ctypes.data, 1, raw_desc(4, 4), p, 64, None, p, p, p) == -1
