"""CPU: the n-tuple network code of g2048_device.h -- the header the kernels are compiled from -- built for the host
(tests/host_ntuple/ntuple_check.cpp, g++) and compared bit for bit with the pure-Python reference tests/ntuple_ref.py.
Every test shows from the reference's own trace (never from the code under test) that its input reaches the edge it
names."""
import numpy as np
import pytest

import ntuple_ref as ref
from analysis_helpers import ONE_LEGAL, TERMINAL, random_boards, trajectory_boards
from move_lut import build_row_lut
from ntuple_helpers import (TUPLES_2x6, TUPLES_8x6, TUPLES_17x4, assert_eval_equal, host_evaluate, host_update, host_values,
                            load_host_ntuple, random_net, raw_desc)

INT32_MAX, INT32_MIN = (1 << 31) - 1, -(1 << 31)


@pytest.fixture(scope="module")
def hn():
    return load_host_ntuple()


def check(lib, boards, net):
    """host == reference for evaluate and values; returns the reference's evaluate."""
    want = ref.evaluate_batch(boards, net)
    assert_eval_equal(host_evaluate(lib, boards, net), want, boards)
    assert np.array_equal(host_values(lib, boards, net), ref.values_batch(boards, net))
    return want


def check_update(lib, boards, deltas, lr_shift, net):
    """host == reference for one update; returns (the new weights, the reference's trace)."""
    after, trace = net.copy(), {}
    ref.update(after, boards, deltas, lr_shift, trace)
    got = host_update(lib, boards, deltas, lr_shift, 0, net)[0]
    bad = np.argwhere(got != after.weights)
    assert len(bad) == 0, f"{len(bad)} weights differ, first {bad[0].tolist()}: {got[tuple(bad[0])]} vs {after.weights[tuple(bad[0])]}"
    return after.weights, trace


def test_shift_row_is_the_row_table(oracle_lib):
    """The reference's move rule equals the oracle's shift() on every row of exponents 0..17 (tests/move_lut.py)."""
    out, score = build_row_lut(oracle_lib)
    rows = np.array(np.meshgrid(*[np.arange(18)] * 4, indexing="ij")).reshape(4, -1).T
    for k in range(0, len(rows), 7):
        new, s = ref.shift_row(tuple(int(x) for x in rows[k]))
        assert list(new) == out[k].tolist() and s == score[k], rows[k]


def test_symmetry_maps_are_the_eight_of_augment(hn):
    """The header applies the symmetries to the cell lists: its eight maps are, as a set, the eight boards numpy's flip
    and rot90 make of the board of cell numbers."""
    maps = np.zeros((8, 16), np.uint8)
    hn.ntuple_check_sym_cells(maps.ctypes.data)
    want = {tuple(p) for p in ref.symmetries(tuple(range(16)))}
    assert len(want) == 8 and {tuple(int(c) for c in m) for m in maps} == want


@pytest.mark.parametrize("tuples", [TUPLES_17x4, TUPLES_2x6], ids=["17x4", "2x6"])
def test_random_and_trajectory_boards(hn, tuples):
    net = random_net(tuples, 1)
    boards = np.concatenate([random_boards(60, 2), trajectory_boards(every=211)[:60]])
    val, act, best, after, av = check(hn, boards, net)
    legal = val != ref.ILLEGAL
    assert legal.any(1).sum() > 100 and (~legal).any()                 # nearly every board can move, some moves are illegal
    assert len(set(act.tolist())) == 4                                 # each direction is somebody's best move
    assert (val[legal] < 0).any() and (val[legal] > 0).any()           # q of both signs
    can = legal.any(1)
    assert (best[can] == val[can, act[can]]).all() and (best[~can] == 0).all() and np.abs(av).max() > 1 << 32


def test_symmetric_board_counts_an_entry_twice(hn):
    """A board equal to its horizontal flip: the reference reads some (tuple, index) entries twice."""
    half = np.random.default_rng(3).integers(0, 12, size=(4, 2))
    board = np.concatenate([half, half[:, ::-1]], axis=1).reshape(1, 16).astype(np.uint8)
    net = random_net(TUPLES_17x4, 4)
    hits = []
    ref.value(ref.plain(board), net, hits)
    assert len(hits) == 8 * 5 and len(set(hits)) < len(hits)
    assert ref.symmetries(ref.plain(board))[0] == ref.symmetries(ref.plain(board))[1]   # board == hflip(board)
    check(hn, board, net)
    # a weight read twice enters V twice: raising it by 1 raises V by its multiplicity
    t, i = next(h for h in hits if hits.count(h) >= 2)
    bumped = net.copy()
    bumped.weights[t, i] += 1 if bumped.weights[t, i] < INT32_MAX else -1
    d = host_values(hn, board, bumped)[0] - host_values(hn, board, net)[0]
    assert abs(d) == hits.count((t, i)) >= 2


def test_exponents_at_and_past_the_clamp(hn):
    """Exponents 15, 16, 17 and 31 share the last table row, 32 + e reads as e; 14 does not share it."""
    assert [ref.cell(e) for e in (14, 15, 16, 17, 31, 32, 33, 47)] == [14, 15, 15, 15, 15, 0, 1, 15]
    net = random_net(TUPLES_17x4, 5)
    base = random_boards(12, 6, max_exp=12)
    boards = []
    for b in base:
        for e in (14, 15, 16, 17, 31, 33, 47):
            x = b.copy()
            x[[0, 5, 10, 15]] = [e, 3, e, 2]     # cells of the corner, the edge and the centre square and of both rows
            boards.append(x)
    boards = np.array(boards, np.uint8)
    val, *_ = check(hn, boards, net)
    v = ref.values_batch(boards, net).reshape(len(base), 7)
    assert (v[:, 1] == v[:, 2]).all() and (v[:, 1] == v[:, 3]).all() and (v[:, 1] == v[:, 4]).all() and (v[:, 1] == v[:, 6]).all()
    assert (v[:, 0] != v[:, 1]).all() and (v[:, 5] != v[:, 1]).all()
    # the afterstates keep their own exponents: the chosen afterstate of a 16-board holds a 16, not a 15
    after = ref.evaluate_batch(boards, net)[3].reshape(len(base), 7, 16)
    assert (after[:, 2] == 16).any() and (after[:, 4] == 31).any()


def test_all_negative_weights(hn):
    """q < 0 for every legal move: the action must still be a legal move, the best q a negative number."""
    net = random_net(TUPLES_17x4, 7, lo=-(1 << 31), hi=-(1 << 29))
    boards = np.concatenate([random_boards(40, 8), ONE_LEGAL])
    val, act, best, _, _ = check(hn, boards, net)
    legal = val != ref.ILLEGAL
    can = legal.any(1)
    assert (val[legal] < 0).all() and (best[can] < 0).all() and legal[can, act[can]].all() and can.sum() > 30
    assert (~legal[:, 0]).any() and act[-1] == 2                        # move 0 is illegal somewhere: the action is not 0 there


def test_equal_q_takes_the_smallest_direction(hn):
    net = ref.Net(TUPLES_17x4, 10)                                      # zero weights: q = gain << F
    pair = np.array([[1, 1] + [0] * 14], np.uint8)                      # up illegal, right and left merge (4), down slides (0)
    lone = np.array([[0] * 5 + [3] + [0] * 10], np.uint8)               # every move legal with gain 0
    val, act, best, _, _ = check(hn, np.concatenate([pair, lone]), net)
    assert val[0].tolist() == [ref.ILLEGAL, 4 << 10, 0, 4 << 10] and act[0] == 1 and best[0] == 4 << 10
    assert val[1].tolist() == [0, 0, 0, 0] and act[1] == 0


def test_one_legal_and_terminal(hn):
    net = random_net(TUPLES_2x6, 9)
    val, act, best, after, av = check(hn, np.concatenate([ONE_LEGAL, TERMINAL]), net)
    assert act[0] == 2 and (val[0, [0, 1, 3]] == ref.ILLEGAL).all() and best[0] == val[0, 2] != ref.ILLEGAL
    assert not np.array_equal(after[0], ONE_LEGAL[0])
    assert act[1] == 0 and best[1] == 0 and av[1] == 0 and (val[1] == ref.ILLEGAL).all() and np.array_equal(after[1], TERMINAL[0])


def test_update_floors_negative_deltas(hn):
    """-5 >> 1 is -3 (floor), not -2 (truncation) and not a large positive number (logical shift)."""
    assert [ref.step_of(d, 1) for d in (-5, 5, -1, 1)] == [-3, 2, -1, 0]
    for d, s in ((-5, 1), (5, 1), (-1, 1), (1, 1), (-1, 40), (-(1 << 40) - 1, 40), (-(1 << 62), 31), (1 << 62, 32)):
        assert hn.ntuple_check_step(d, s) == ref.step_of(d, s), (d, s)
    net = random_net(TUPLES_17x4, 10, lo=-1000, hi=1000)
    boards = random_boards(8, 11)
    new, trace = check_update(hn, boards, [-5, 5, -1, 1, -7, 0, -(1 << 20) - 1, 3], 1, net)
    assert trace["zero"] == 2 and trace["sat"] == 0 and (new != net.weights).any()


def test_update_saturates_at_both_ends(hn):
    assert ref.step_of(1 << 40, 0) == INT32_MAX and ref.step_of(-(1 << 40), 0) == INT32_MIN
    assert ref.step_of((1 << 31) << 7, 7) == INT32_MAX and ref.step_of(-(1 << 31) << 7, 7) == INT32_MIN   # the first to clip / the last to fit
    net = ref.Net(TUPLES_2x6, 10)
    boards = random_boards(4, 12)
    new, trace = check_update(hn, boards, [1 << 40, -(1 << 40), (1 << 31) << 7, -(1 << 31) << 7], 7, net)
    assert trace["sat"] == 3 and (new != 0).any()                       # -(2^31) is the one step that fits


def test_update_wraps_a_weight_at_int32_max(hn):
    net = ref.Net(TUPLES_17x4, 10)
    net.weights[:] = INT32_MAX
    board = random_boards(1, 13)
    new, trace = check_update(hn, board, [1], 0, net)
    assert trace["wrap"] > 0 and new.min() <= INT32_MIN + 8 and (new == INT32_MAX).any()


def test_update_with_duplicate_boards(hn):
    """The same board several times in one batch: its entries collect every step."""
    net = random_net(TUPLES_17x4, 14, lo=-1000, hi=1000)
    b = random_boards(3, 15)
    boards = np.concatenate([b, b[:1], b[:1], b[1:2]])
    deltas = [64, -128, 192, 64, 640, 256]
    new, _ = check_update(hn, boards, deltas, 6, net)
    once = net.copy()
    ref.update(once, b, [1 + 1 + 10, -2 + 4, 3], 0)
    assert np.array_equal(new, once.weights)


@pytest.mark.parametrize("tuples", [((9,),), TUPLES_8x6], ids=["T1L1", "T8L6"])
def test_smallest_and_largest_shape(hn, tuples):
    """T = 1, L = 1 and T = 8, L = 6; a board of 15s and above reads and updates the last entry of the last table."""
    net = random_net(tuples, 16)
    T, size = len(tuples), 16 ** len(tuples[0])
    top = np.array([[15, 16, 17, 31] * 4], np.uint8)
    hits = []
    ref.value(ref.plain(top), net, hits)
    assert (T - 1, size - 1) in hits and all(i == size - 1 for _, i in hits)
    boards = np.concatenate([top, random_boards(20, 17)])
    check(hn, boards, net)
    new, _ = check_update(hn, boards, np.arange(1, 22) * 1000, 3, net)
    assert new[T - 1, size - 1] != net.weights[T - 1, size - 1]


def test_shapes_out_of_range_are_refused(hn):
    z = np.zeros(64, np.int64)
    p = z.ctypes.data
    for T, L, F in ((0, 4, 10), (9, 4, 10), (4, 0, 10), (4, 7, 10), (4, 4, 17)):
        assert hn.ntuple_check_evaluate(p, 1, raw_desc(T, L, F), p, p, p, p, p, p) == -1
    assert hn.ntuple_check_update(p, 1, p, 41, 0, raw_desc(4, 4), p, p, p) == -1
