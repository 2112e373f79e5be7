"""GPU: every instantiation of the two n-tuple search kernels that a network can reach -- ntuple_search_kernel (depths 1 and
2) and ntuple_deep_search_kernel (depths 2 and 3) over the tuple counts T = 1..8, the three shape types and the three launch
forms -- against the pure-Python references (ntuple_search_ref, ntuple_staged_ref on the padded array of ntuple_mixed_ref), bit
for bit.  Every test shows from the reference or the definition (never from the code under test) that its input reaches the
edge it names.

Three families of networks (ntuple_deep_helpers.family_net), full-range random int32 weights, F = 10.  Network T of a family
has the first T cell lists and the first T tables (of every stage) of the family's network 8, so the reference's outputs for
T - 1 are those of a launch that took the neighbouring instantiation: they must differ, and every test asserts it.
  uniform  TUPLES_8x4[:T], T = 1..8                                       NtupleShape
  staged   TUPLES_8x4[:T] on LOW_THR[:2] (S = 3), T = 1..8                NtupleStagedShape
  mixed    ntuple_mixed_ref.MIX_8[:T] on LOW_THR[:2] (S = 3), T = 2..8    NtupleMixedShape (lengths 4, 1, 3, 2, 4, 2, 3, 1)

Reached, per (family, T) -- 23 networks; "3 forms" = plain boards, engine records, engine records with an ``active`` mask (all
non-zero in different words; alternating; the other alternation):
  kernel                      depth  forms  boards                                              expected values from
  ntuple_search_kernel        1      3      boards_64                                           the reference
  ntuple_search_kernel        2      3      near_full_12 + LOW_STAGE (14)                       the reference
  ntuple_deep_search_kernel   2      3      the same 14 + the one-tile board WIDE_FANS[0]       the reference; search(.., 2) for the last
  ntuple_deep_search_kernel   3      3      near_full(2) boards, PAIR_ONLY, TERMINAL,           compose_depth3 over search(.., 2), which the
                                            WIDE_FANS[0], LOW_STAGE[0] (10)                     depth-2 test ties to the reference
  ntuple_deep_search_kernel   3      3      near_full(2) boards, uniform T = 8 only             the pure-Python depth-3 reference
  evaluate, values            -      2, 1   boards_64, staged and mixed (uniform: test_gpu_ntuple_shapes.py)   the reference
That is 23 * 2 * 3 = 138 instantiations of each kernel, 276 of the 288 compiled.  NOT reached: the mixed shape at T = 1, 6
kernels of each (2 depths * 3 forms), 12 in all.  NTupleNet takes tuple_len from the longest list, so a network of one list is
never mixed and no call can select them.

LOW_STAGE: near_full_12 alone keeps every depth-2 leaf in the last stage (its boards hold tiles of 8 and more, and the low
thresholds ask for a 4 and an 8), so two near-full boards of 2s and 4s are added: their leaves lie in two stages, which the
tests assert from the reference's trace.

CPU time of the reference work per (family, T), measured on one core with the tests' own inputs, T = 1 (2 for mixed) .. 8; it
is cached per module, the device work is milliseconds:
  uniform  search depth 1: 0.6 .. 1.6 s    depth 2: 0.6 .. 3.2 s
  staged   search depth 1: 0.6 .. 2.0 s    depth 2: 0.4 .. 1.6 s    evaluate and values: below 0.1 s
  mixed    search depth 1: 0.7 .. 1.9 s    depth 2: 0.6 .. 1.9 s    evaluate and values: below 0.1 s
  uniform T = 8, depth 3, the six boards of near_full(2) (0 or 1 empty cell each): 15 s, once per module
On the MI355X's host the whole module takes 33 s; its slowest test is the depth-3 reference (5.6 s), every other below 1 s.

Tried once on scratch builds of the library (never committed): with dispatch_tuples sending T = 5 to the instantiation of T = 4,
the search kernel (both depths), evaluate and values and the deep kernel at depth 2 fail at T = 5 in every family and nothing
else fails (the composition at depth 3 moves with its depth-2 calls: it guards the deep kernel's own dispatch, not the shared
one); with the MASKED deep kernel ignoring o.active, every deep test fails at the alternating mask and no other test does.
"""
import numpy as np
import pytest

import ntuple_search_ref as sref
import ntuple_staged_ref as stref
from analysis_helpers import TERMINAL, g  # noqa: F401 (g: fixture)
from ntuple_deep_helpers import (FAMILIES, ILLEGAL, LOW_STAGE, cached, children_of, compose_depth3, dev, dev_u32, device_net, engine_with,
                                 family_net, kind_of, near_full, to_np)
from ntuple_helpers import assert_eval_equal
from ntuple_mixed_helpers import boards_67, near_full_12
from ntuple_search_helpers import PAIR_ONLY, WIDE_FANS, assert_search_equal

pytestmark = pytest.mark.gpu

CASES = [(family, T) for family, counts in FAMILIES.items() for T in counts]
STAGED_CASES = [(family, T) for family, T in CASES if family != "uniform"]
MASK_WORDS = (1, 7, 1 << 31, 0xffffffff)     # what "active" looks like: any non-zero word


def case_id(case):
    return f"{case[0]}-{case[1]}"


def boards_64():
    """The 64 boards of tests/test_gpu_ntuple_shapes.py: 60 mixed boards, the tie board, PAIR_ONLY, ONE_LEGAL and TERMINAL."""
    return boards_67()[:64]


def boards_14():
    """The 12 near-full boards of tests/test_gpu_ntuple_shapes.py and the two of LOW_STAGE."""
    return cached("matrix depth 2", lambda: np.concatenate([near_full_12(), LOW_STAGE]))


def boards_10():
    """Depth 3: the six boards of near_full(2), PAIR_ONLY, TERMINAL, the one-tile board and a board of 2s and 4s."""
    return cached("matrix depth 3", lambda: np.concatenate([near_full(2)[0], PAIR_ONLY, TERMINAL, WIDE_FANS[:1], LOW_STAGE[:1]]))


def searched(family, T, depth):
    """((action, value), trace) of the reference at depth 1 on boards_64 or at depth 2 on boards_14, once per network: an
    ntuple_search_ref.Trace for the uniform family, the staged reference's dict of counters for the others."""
    def make():
        net, boards = family_net(family, T), boards_64() if depth == 1 else boards_14()
        if kind_of(net) == 0:
            trace = sref.Trace()
            return sref.search_batch(boards, depth, net, trace), trace
        trace = {"memo": {}}
        return stref.search_batch(boards, depth, net, trace), trace
    return cached(("matrix search", family, T, depth), make)


def evaluated(family, T):
    """(evaluate's five outputs, values, evaluate's trace, values' trace) of the staged reference on boards_64."""
    def make():
        net, te, tv = family_net(family, T), {}, {}
        return stref.evaluate_batch(boards_64(), net, te), stref.values_batch(boards_64(), net, tv), te, tv
    return cached(("matrix evaluate", family, T), make)


def assert_inputs(family, T, depth):
    """What the reference says about the depth-``depth`` case of network T: the edges its boards reach, and that network
    T - 1 of the family gives other numbers."""
    (act, val), trace = searched(family, T, depth)
    boards = boards_64() if depth == 1 else boards_14()
    legal = val != ILLEGAL
    assert (val[63 if depth == 1 else 11] == ILLEGAL).all() and legal.all(1).any(), "inputs: TERMINAL, and a board with four legal moves"
    assert len(set(act.tolist())) >= 3 and (np.abs(val[legal]) < 1 << 50).all()
    if family == "uniform":
        assert trace.negative_inexact > 0 and trace.terminal_children >= 2
    else:
        thr, on_boards = family_net(family, T).thr, {}
        stref.stage_batch(boards, thr, on_boards)
        assert len(on_boards["stage"]) >= 2, "inputs: the boards lie in at least two stages"
        assert len(trace["stage"]) >= 2, "inputs: the leaves lie in at least two stages"
        assert trace["leaf_other"] > 0, "inputs: leaves in another stage than their root board"
    if T > 1:   # (mixed, 1) is a reference network only: one list cannot be mixed on the device
        assert (searched(family, T - 1, depth)[0][1] != val).any(), "the neighbouring instantiation computes something else"


def check_three_forms(g, torch, boards, want, plain, engine, where):
    """``plain(device boards)``, ``engine(eng, None)`` and ``engine(eng, active)`` against ``want``: the masked form with every
    board on (different non-zero words) and with every other board off, in both alternations -- a board that is off gets action
    0 and four ILLEGAL.  The engine's records and clock and the mask are left as they were."""
    n = len(boards)
    assert_search_equal(to_np(plain(dev(torch, boards))), want, boards, f"{where}, plain")
    eng = engine_with(g, boards)
    try:
        rec, clock = eng.records().clone(), eng.clock
        assert bool((rec[:, 8:] > 31).any()), "inputs: the score-deficit bits are populated"
        assert_search_equal(to_np(engine(eng, None)), want, boards, f"{where}, engine")
        words = np.array(MASK_WORDS, np.uint32)[np.arange(n) % 4]
        assert_search_equal(to_np(engine(eng, dev_u32(torch, words))), want, boards, f"{where}, masked, all on")
        for parity in (0, 1):
            on = np.arange(n) % 2 == parity
            mask = np.where(on, words, 0).astype(np.uint32)
            active = dev_u32(torch, mask)
            act, val = to_np(engine(eng, active))
            assert_search_equal((act[on], val[on]), (want[0][on], want[1][on]), boards[on], f"{where}, masked, parity {parity}, active rows")
            assert not act[~on].any() and (val[~on] == ILLEGAL).all(), f"{where}, masked, parity {parity}, inactive rows"
            assert np.array_equal(active.view(torch.int32).cpu().numpy().view(np.uint32), mask)
        assert torch.equal(eng.records(), rec) and eng.clock == clock
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ ntuple_search_kernel
@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_search_kernel_equals_the_reference_in_three_forms(g, torch_cuda, case, depth):
    family, T = case
    assert_inputs(family, T, depth)
    boards = boards_64() if depth == 1 else boards_14()
    assert depth == 1 or ((boards == 0).sum(1) <= 2).all()
    net = device_net(g, family_net(family, T))
    assert net.n_tuples == T and (net.mixed, net.n_stages) == {"uniform": (False, 1), "staged": (False, 3), "mixed": (True, 3)}[family]
    check_three_forms(g, torch_cuda, boards, searched(family, T, depth)[0], lambda d: net.search(d, depth),
                      lambda eng, active: eng.ntuple_search(net, depth, active=active), f"{family} T={T} depth {depth}")


# ------------------------------------------------------------------------------------------------ evaluate, values
@pytest.mark.parametrize("case", STAGED_CASES, ids=case_id)
def test_evaluate_and_values_of_staged_and_mixed_networks(g, torch_cuda, case):
    torch = torch_cuda
    family, T = case
    boards = boards_64()
    want_e, want_v, te, tv = evaluated(family, T)
    assert len(te["stage"]) >= 2 and len(tv["stage"]) == 3, "inputs: afterstates in two stages, boards in all three"
    assert (want_e[0][63] == ILLEGAL).all() and len(set(want_e[1].tolist())) == 4
    if T > 1:
        prev_e, prev_v, _, _ = evaluated(family, T - 1)
        assert (prev_e[0] != want_e[0]).any() and (prev_e[4] != want_e[4]).any() and (prev_v != want_v).any()
    net, d = device_net(g, family_net(family, T)), dev(torch, boards)
    assert_eval_equal(to_np(net.evaluate(d)), want_e, boards, "evaluate, plain")
    assert np.array_equal(net.values(d).cpu().numpy(), want_v), "values"
    eng = engine_with(g, boards)
    try:
        rec, clock = eng.records().clone(), eng.clock
        assert_eval_equal(to_np(eng.ntuple_evaluate(net)), want_e, boards, "evaluate, engine")
        assert torch.equal(eng.records(), rec) and eng.clock == clock
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ ntuple_deep_search_kernel
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_deep_kernel_at_depth_2_equals_the_reference_in_three_forms(g, torch_cuda, case):
    """The 14 boards of the depth-2 reference and the one-tile board (four legal moves onto 15 empty cells: 120 level-1 items),
    whose row comes from search(.., 2) -- the kernel the test above ties to the reference for this very network."""
    torch = torch_cuda
    family, T = case
    assert_inputs(family, T, 2)
    wide = WIDE_FANS[:1]
    items, _, empties = children_of(wide)
    assert [len(lst) for lst in items[0]] == [30] * 4 and empties[0] == [15] * 4
    net = device_net(g, family_net(family, T))
    ref_act, ref_val = searched(family, T, 2)[0]
    wide_act, wide_val = to_np(net.search(dev(torch, wide), 2))
    assert (wide_val != ILLEGAL).all()
    want = np.concatenate([ref_act, wide_act]), np.concatenate([ref_val, wide_val])
    check_three_forms(g, torch, np.concatenate([boards_14(), wide]), want, lambda d: net.deep_search(d, 2),
                      lambda eng, active: eng.ntuple_deep_search(net, 2, active=active), f"{family} T={T} deep, depth 2")


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_deep_kernel_at_depth_3_equals_the_composition_in_three_forms(g, torch_cuda, case):
    """value[d] = (g << F) + (sum of w * S_2(child)) // (10 E) with S_2 from search(.., 2) of this network."""
    torch = torch_cuda
    family, T = case
    boards = boards_10()
    rnet = family_net(family, T)
    net = device_net(g, rnet)
    want, widest, dead = compose_depth3(boards, rnet.frac_bits, lambda kids: net.search(dev(torch, kids), 2).value.cpu().numpy())
    items = children_of(boards)[0]
    assert sum(len(lst) for lst in items[8]) == 120, "inputs: the one-tile board fills the table, 120 items and 480 entries"
    assert widest == 30 and dead >= 1, "inputs: a direction with 30 level-1 items, a child with no legal move"
    legal = want[1] != ILLEGAL
    assert legal[8].all() and not legal[7].any() and (np.abs(want[1][legal]) < 1 << 50).all()
    check_three_forms(g, torch, boards, want, lambda d: net.deep_search(d, 3), lambda eng, active: eng.ntuple_deep_search(net, 3, active=active),
                      f"{family} T={T} deep, depth 3")


def test_deep_kernel_at_depth_3_equals_the_reference_for_8_tuples(g, torch_cuda):
    """T = 8 at depth 3 against a reference that passes through no kernel: the six boards of near_full(2), uniform network 8."""
    boards, rnet = near_full(2)[0], family_net("uniform", 8)

    def make():
        trace = sref.Trace()
        return sref.search_batch(boards, 3, rnet, trace), trace
    want, trace = cached("matrix depth 3 reference", make)
    assert len(boards) == 6 and ((boards == 0).sum(1) <= 2).all() and len(rnet.tuples) == 8
    assert trace.chance > 4000 and trace.negative_inexact > 200 and trace.terminal_children > 30
    assert (want[1] != ILLEGAL).any(1).all() and (want[1] != sref.search_batch(boards, 2, rnet)[1]).any()
    net = device_net(g, rnet)
    check_three_forms(g, torch_cuda, boards, want, lambda d: net.deep_search(d, 3), lambda eng, active: eng.ntuple_deep_search(net, 3, active=active),
                      "uniform T=8 deep, depth 3, reference")
