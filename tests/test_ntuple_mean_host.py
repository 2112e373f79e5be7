"""CPU: the batch-mean n-tuple update (include/g2048.h "Batch-mean update") without a GPU -- the header's two
per-item operations, ntuple_item_mean_sum and ntuple_item_mean_apply, built with g++ (tests/host_ntuple_mean: plain adds, a plain
exchange) against the pure-Python reference tests/ntuple_mean_ref.py, bit for bit and as whole arrays.  Every call runs its items
forward, in reverse and shuffled, and the three must agree: the order-independence claim of the definition.  Every test shows
first, from the reference alone, that its input reaches the edge it names.  After every phases=3 call sum and count are zero.
Fails on the parent commit: the header has no such operations."""
import numpy as np
import pytest

import ntuple_mean_ref as meanref
import ntuple_mixed_ref as mref
import ntuple_ref as ref
import ntuple_staged_ref as sref
import ntuple_update_matrix as um
from analysis_helpers import mixed_boards
from ntuple_helpers import TUPLES_8x4
from ntuple_mean_helpers import (KIND, assert_matrix_conditions, assert_mean_tables, host_trace_update, host_update, load_host_mean,
                                 matrix_case, mean_of, mean_update_np, orders, trace_items_np, want_tables)
from ntuple_mixed_helpers import THR_3

EMPTY, SAME = [0] * 16, [3] * 16                 # one entry per table, reached by all 8 symmetries
TUPLES_3 = tuple(TUPLES_8x4[:3])


@pytest.fixture(scope="module")
def lib():
    return load_host_mean()


def fresh(tuples=TUPLES_3, thr=(), seed=7):
    net = um.ref_net(tuples, seed, thr)
    return net, meanref.Mean(net)


def state_from(got, like):
    """(network, state) holding the compact flat tables ``got`` = (weights, sum, count)."""
    S = like.n_stages
    net = mref.mixed_net(like.tuples, like.thr, like.frac_bits, got[0].reshape(S, -1))
    return net, mean_of(net, got[1], got[2])


def run_all_orders(lib, boards, deltas, lr_shift, net, mean, kind=2, trace=None):
    """The reference's tables after a phases=3 call, after checking the host build against them in three item orders, and that
    the reference itself does not depend on the order."""
    rnet, rmean = net.copy(), mean.copy()
    meanref.mean_update(rnet, rmean, boards, deltas, lr_shift, 3, trace)
    want = want_tables(rnet, rmean)
    assert rmean.is_zero() or not mean.is_zero()
    for name, order in zip(("forward", "reverse", "shuffled"), orders(len(deltas))):
        assert_mean_tables(host_update(lib, boards, deltas, lr_shift, 3, net, mean, order, kind), want, f"{name}: ")
        if order is not None:
            onet, omean = net.copy(), mean.copy()
            meanref.mean_update(onet, omean, boards, deltas, lr_shift, 3, order=list(order))
            assert_mean_tables(want_tables(onet, omean), want, f"reference, {name}: ")
    return want


def moved(want, net):
    """{compact element: change of the weight} of the entries that changed."""
    base = mref.flat_of(net).reshape(-1)
    idx = np.nonzero(want[0] != base)[0]
    return {int(i): int(want[0][i] - base[i]) for i in idx}


def test_floor_div_floors(lib):
    import ctypes as C
    out = C.c_int64()
    for a, c in ((-7, 2), (7, 2), (-8, 2), (-1, 3), (0, 5), (-(1 << 63), 1), (-(1 << 63), 3), ((1 << 63) - 1, (1 << 32) - 8), (-1, (1 << 32) - 1)):
        assert lib.mean_check_floor_div(a, c, C.addressof(out)) == 0 and out.value == meanref.floor_div(a, c) == a // c, (a, c)
    assert meanref.floor_div(-7, 2) == -4


@pytest.mark.parametrize("family", ["uniform", "staged", "mixed"])
def test_entries_reached_by_several_boards(lib, family):
    T = {"uniform": 3, "staged": 2, "mixed": 4}[family]
    net, _ = um.family_net(family, T)
    mean, trace = meanref.Mean(net), {}
    boards, deltas = um.pool()[0], um.board_case(family, T).deltas
    want = run_all_orders(lib, boards, deltas, 3, net, mean, KIND[family], trace)
    assert trace["multi"] > 0 and trace["max_count"] > 2 and trace["neg_rem"] > 0 and trace["zero"] > 0 and trace["clamp_d"] > 0
    assert not want[1].any() and not want[2].any()
    if family != "mixed":                                            # lists of one length: the mixed shape type gives the same
        assert_mean_tables(host_update(lib, boards, deltas, 3, 3, net, mean, None, 2), want, "as a mixed shape: ")


def test_a_symmetric_board_moves_each_weight_by_one_step(lib):
    for board in (EMPTY, SAME):
        net, mean = fresh()
        trace, delta, lr = {}, 1000, 2
        want = run_all_orders(lib, [board], [delta], lr, net, mean, 0, trace)
        T = len(net.tuples)
        assert trace["entries"] == T and trace["sym"] == T and trace["by_table"] == {(0, t): 8 for t in range(T)} and trace["multi"] == 0
        assert moved(want, net) == {e: ref.step_of(delta, lr) for e in set(mref.lookups(board, net))}
        plain = net.copy()
        sref.update(plain, [board], [delta], lr)                     # the summed update: 8 steps
        assert moved((mref.flat_of(plain).reshape(-1),), net) == {e: 8 * ref.step_of(delta, lr) for e in set(mref.lookups(board, net))}
        assert not want[1].any() and not want[2].any()


def some_board(n=1, seed=3):
    return mixed_boards(n, seed)


def test_a_negative_sum_its_count_does_not_divide_is_floored(lib):
    net, mean = fresh()
    b, trace = some_board()[0], {}
    want = run_all_orders(lib, [b, b], [-3, -4], 0, net, mean, 0, trace)
    assert trace["neg_rem"] == trace["entries"] > 0
    assert set(moved(want, net).values()) == {-4}                    # floor(-7 / 2) and floor(-14 / 4): -4, not -3
    assert set(moved(want, net)) == set(mref.lookups(b, net))


def test_errors_that_cancel_leave_the_weight_and_clear_the_state(lib):
    net, mean = fresh()
    b, trace = some_board()[0], {}
    want = run_all_orders(lib, [b, b], [5, -5], 0, net, mean, 0, trace)
    assert trace["cancel"] == trace["entries"] > 0 and trace["moved"] == 0
    assert_mean_tables(want, want_tables(net, mean))                 # nothing moved, and sum and count are zero again


def test_a_mean_that_is_not_zero_can_have_a_zero_step(lib):
    net, mean = fresh()
    b, trace = some_board()[0], {}
    want = run_all_orders(lib, [b, b], [5, 6], 10, net, mean, 0, trace)
    assert trace["zero_step"] == trace["entries"] > 0
    assert_mean_tables(want, want_tables(net, mean))
    trace = {}
    want = run_all_orders(lib, [b, b], [-5, -6], 10, net, mean, 0, trace)   # the shift floors: floor(-11 / 2) >> 10 = -1
    assert set(moved(want, net).values()) == {-1} and trace["zero_step"] == 0


def test_deltas_beyond_the_clamp_are_clamped(lib):
    net, mean = fresh()
    boards = some_board(4, 8)
    deltas, trace = [(1 << 40) + 1, -(1 << 40) - 1, (1 << 63) - 1, -(1 << 63)], {}
    want = run_all_orders(lib, boards, deltas, 20, net, mean, 0, trace)
    assert trace["clamp_d"] == 4 and trace["sat"] == 0
    clamped = net.copy()
    cm = meanref.Mean(clamped)
    meanref.mean_update(clamped, cm, boards, [1 << 40, -(1 << 40), 1 << 40, -(1 << 40)], 20)
    assert_mean_tables(want, want_tables(clamped, cm))


def test_a_mean_of_2_31_or_more_saturates(lib):
    net, mean = fresh()
    b, trace = some_board()[0], {}
    want = run_all_orders(lib, [b, b], [1 << 40, 1 << 31], 0, net, mean, 0, trace)
    assert trace["sat"] == trace["entries"] > 0
    base = mref.flat_of(net).reshape(-1)
    for e in set(mref.lookups(b, net)):
        assert want[0][e] == ref.wrap32(int(base[e]) + ref.INT32_MAX)
    want = run_all_orders(lib, [b], [-(1 << 40)], 0, net, mean, 0)
    for e in set(mref.lookups(b, net)):
        assert want[0][e] == ref.wrap32(int(base[e]) + ref.INT32_MIN)


def test_zero_deltas_touch_nothing(lib):
    net, mean = fresh()
    rng = np.random.default_rng(4)
    mean.sum[:] = rng.integers(-(1 << 62), 1 << 62, size=mean.sum.shape)        # pending state: a zero item may not even claim it
    mean.count[:] = rng.integers(1, 1 << 32, size=mean.count.shape, dtype=np.uint64).astype(np.uint32)
    boards = some_board(5, 9)
    for phases in (1, 2, 3):
        for order in orders(5):
            assert_mean_tables(host_update(lib, boards, [0] * 5, 0, phases, net, mean, order, 0), want_tables(net, mean), f"phases {phases}: ")
    trace = {}
    meanref.mean_update(net.copy(), mean.copy(), boards, [0] * 5, 0, 3, trace)
    assert trace["zero"] == 5 and trace["entries"] == 0


def disjoint_boards(net, n):
    """n boards none of whose look-ups coincide, within a board or between two: from the reference's look-ups alone."""
    seen, out = set(), []
    for b in mixed_boards(200, 21):
        hits = mref.lookups(b, net)
        if len(set(hits)) == len(hits) and not seen & set(hits):
            seen |= set(hits)
            out.append(b)
            if len(out) == n:
                return np.array(out, np.uint8)
    raise AssertionError("inputs: not enough disjoint boards")


def test_disjoint_entries_give_the_plain_update(lib):
    net, mean = fresh()
    boards = disjoint_boards(net, 12)
    deltas = [((-1) ** i) * ((i + 1) << (3 * i)) for i in range(12)]             # up to 12 << 33: below the clamp
    trace = {}
    want = run_all_orders(lib, boards, deltas, 5, net, mean, 0, trace)
    assert trace["multi"] == 0 and trace["sym"] == 0 and trace["max_count"] == 1 and max(abs(d) for d in deltas) <= 1 << 40
    plain = net.copy()
    sref.update(plain, boards, deltas, 5)
    assert np.array_equal(want[0], mref.flat_of(plain).reshape(-1)) and trace["moved"] > 0


def test_copies_of_one_item_give_one_copy(lib):
    net, mean = fresh(tuple(mref.MIX_8[:4]), THR_3)
    boards, deltas = um.pool()[1][:9], [-700, 33, 1 << 20, -5, 0, 9, -(1 << 30), 77, 1]
    one = run_all_orders(lib, boards, deltas, 3, net, mean)
    for c in (2, 5):
        assert_mean_tables(run_all_orders(lib, np.tile(boards, (c, 1)), deltas * c, 3, net, mean), one, f"{c} copies: ")


def test_shards_sum_everywhere_then_apply_everywhere(lib):
    net, mean = fresh(TUPLES_3, THR_3)
    boards, deltas = um.pool()[2], um.board_case("staged", 3).deltas
    A, B = slice(0, 30), slice(30, 65)
    trace = {}
    whole = run_all_orders(lib, boards, deltas, 3, net, mean, 1, trace)
    shared = set(e for b in boards[A] for e in mref.lookups(b, net)) & set(e for b in boards[B] for e in mref.lookups(b, net))
    assert shared and trace["multi"] > 0                              # the shards meet in some entries
    state = (net, mean)
    for phases, part in ((1, A), (1, B), (2, A)):
        got = host_update(lib, boards[part], deltas[part], 3, phases, *state, None, 1)
        state = state_from(got, net)
    # APPLY on shard A alone: what only B reached is still pending
    rnet, rmean = net.copy(), mean.copy()
    meanref.mean_update(rnet, rmean, boards[A], deltas[A], 3, 1)
    meanref.mean_update(rnet, rmean, boards[B], deltas[B], 3, 1)
    meanref.mean_update(rnet, rmean, boards[A], deltas[A], 3, 2)
    assert_mean_tables(got, want_tables(rnet, rmean), "after APPLY(A): ")
    assert got[2].any() and got[1].any()
    got = host_update(lib, boards[B], deltas[B], 3, 2, *state, None, 1)
    assert_mean_tables(got, whole, "after APPLY(B): ")


def test_apply_alone_on_zero_state_changes_nothing(lib):
    net, mean = fresh()
    boards, deltas = um.pool()[0], um.board_case("uniform", 3).deltas
    assert_mean_tables(host_update(lib, boards, deltas, 3, 2, net, mean, None, 0), want_tables(net, mean))
    rnet, rmean = net.copy(), mean.copy()
    meanref.mean_update(rnet, rmean, boards, deltas, 3, 2)
    assert_mean_tables(want_tables(rnet, rmean), want_tables(net, mean))


def test_sum_then_apply_is_both(lib):
    net, mean = fresh()
    boards, deltas = um.pool()[0], um.board_case("uniform", 3).deltas
    both = host_update(lib, boards, deltas, 3, 3, net, mean, None, 0)
    summed = host_update(lib, boards, deltas, 3, 1, net, mean, None, 0)
    assert np.array_equal(summed[0], mref.flat_of(net).reshape(-1)) and summed[1].any() and summed[2].any()   # SUM leaves the weights
    assert_mean_tables(host_update(lib, boards, deltas, 3, 2, *state_from(summed, net), orders(65)[2], 0), both)


@pytest.mark.parametrize("case", um.CASES, ids=um.case_id)
@pytest.mark.parametrize("source", ["board", "trace"])
def test_update_matrix(lib, case, source):
    """The cases tests/test_gpu_ntuple_mean_matrix.py runs on the device: their expected tables, checked here without one."""
    family, T = case
    assert_matrix_conditions(family, T, source)
    c = matrix_case(family, T, source)
    net, _ = um.family_net(family, T)
    mean = meanref.Mean(net)
    want = c.want.on(um.base_tables(family, T)[:1]) + (np.zeros(1), np.zeros(1))
    n_items = um.N if source == "board" else um.N * um.H
    for name, order in zip(("forward", "reverse", "shuffled"), orders(n_items)):
        if source == "board":
            got = host_update(lib, c.case.boards, c.case.deltas, c.case.lr_shift, 3, net, mean, order, KIND[family])
        else:
            got = host_trace_update(lib, c.case.tr, c.case.deltas, c.case.lr_shift, 3, net, mean, order, KIND[family])
        assert_mean_tables(got[:1], want[:1], f"{name}: ")
        assert not got[1].any() and not got[2].any(), f"{name}: sum and count are not zero after the call"


def test_the_numpy_form_is_the_reference():
    """mean_update_np and trace_items_np (what the GPU tests use for thousands of boards) against the scalar reference, on the 65
    boards and the ring of the update matrix, staged and mixed."""
    for family, T in (("uniform", 3), ("staged", 4), ("mixed", 5)):
        for source in ("board", "trace"):
            c = matrix_case(family, T, source)
            base = um.base_tables(family, T)[0]
            boards, deltas = (c.case.boards, c.case.deltas) if source == "board" else trace_items_np(c.case.tr, c.case.deltas)
            got = mean_update_np(base.copy(), um.family_tuples(family, T), boards, deltas, c.case.lr_shift, um.family_thr(family))
            assert np.array_equal(got, c.want.on((base,))[0]), (family, source)
