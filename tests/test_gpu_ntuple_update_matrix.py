"""GPU: every instantiation of the three n-tuple update kernels that a network can reach -- ntuple_update_kernel,
ntuple_tc_weights_kernel and ntuple_tc_accum_kernel over the tuple counts T = 1..8, the three shape types and the three item
sources -- against the pure-Python references (ntuple_staged_ref and ntuple_delay_ref on the padded array of ntuple_mixed_ref),
bit for bit and as whole arrays: the weights after the TD update; weights, err and mag after the TC update, once as one call with
phases=3 and once as phases=1 then phases=2 on fresh copies; for the delay ring also hist, len, acc and delta after every push,
and the ring unchanged by every update.  There is no tolerance anywhere.

The cases, their inputs and the expected tables are tests/ntuple_update_matrix.py's, which tests/test_ntuple_update_matrix_cpu.py
checks against the host builds of the same item code.  Every test first asserts ntuple_update_matrix.assert_conditions -- from
the references and the inputs, never from the device: the reference changes every one of the T tables in every one of the S
stages, in the weights of both forms and in err and mag (which fails for a launch of the instantiation of T - 1, whose tables the
test also builds and compares, and for a staged or mixed network sent to the uniform shape, which writes stage 0 only); the TC
weights differ from the TD weights; the boards lie in all three stages and, for the trace and the delay, one board's valid slots
lie in different stages; items with step 0, a delta beyond 2^40, boards with fewer than H valid slots, episodes that ended at
the last push are present; the delay applies afterstates in both modes, n * pushes in all.

Three families of networks (ntuple_update_matrix.family_net), full-range random int32 weights, random accumulators, F = 10:
  uniform  TUPLES_8x4[:T], T = 1..8                                     NtupleShape
  staged   TUPLES_8x4[:T] on THR_3 (S = 3), T = 1..8                    NtupleStagedShape
  mixed    ntuple_mixed_ref.MIX_8[:T] on THR_3 (S = 3), T = 2..8        NtupleMixedShape (lengths 4, 1, 3, 2, 4, 2, 3, 1)

Reached, per (family, T) -- 23 networks -- and item source, 65 boards each (one workgroup: a full wave and one lane):
  source             inputs                                                          kernels
  NtupleBoardItems   small_boards, edge_deltas                                       update, tc_weights, tc_accum
  NtupleTraceItems   H = 4, lambda = 0.75, 7 pushes of small_boards, trace_deltas     update, tc_weights, tc_accum
  NtupleDelayItems   the same ring and boards, 7 pushes with a STEP update after      update, tc_weights, tc_accum
                     each and one FLUSH
That is 23 * 3 * 3 = 207 of the 216 compiled kernels (8 tuple counts * 3 shapes * 3 sources * 3 kernels).  NOT reached: the
mixed shape at T = 1, 3 sources * 3 kernels = 9.  NTupleNet takes tuple_len from the longest list, so a network of one list is
never mixed and the Python layer cannot select them (dispatch_tuples would, for a hand-made C descriptor whose only list ends
before tuple_len).

What the suite launched before this module, re-derived from the networks its tests build and from dispatch_tuples (a mixed
descriptor takes NtupleMixedShape whatever S is, any other NtupleStagedShape only for S > 1) -- 107 of the 216:
  uniform  every T over all three sources and kernels: test_gpu_ntuple_shapes.py (board items), test_every_tuple_count of
           test_gpu_ntuple_trace.py and test_gpu_ntuple_delay.py                                                       72 of 72
  staged   T = 5 over board and trace items (TUPLES_17x4 on thresholds: test_gpu_ntuple_staged.py, the trainers, the carousel,
           the uniform side of the equal cut): 6; T = 3 over the delay ring (test_staged_network_whose_pushes_cross_a_stage_
           boundary): 3; T = 8 in the TD kernel over board items (the 4 GiB network of test_gpu_ntuple_staged.py): 1    10 of 72
  mixed    T = 2 ("ext"), 4 ("asc", "desc", the trainers), 5 (the hand-made equal cut of "17x4", against the uniform kernels
           only) and 8 ("8", the preset) over board and trace items: 4 * 6 = 24; over the delay ring the TD kernel at T = 8
           alone (test_mixed_network_4x6_4x4_td): 1                                                                     25 of 72
So 100 kernels that a network can reach were compiled and never run: staged at T = 1, 2, 4, 6, 7 everywhere, at T = 3 and 8
outside the one source or kernel above and at T = 5 over the delay ring; mixed at T = 3, 6, 7 everywhere and at every T over the
delay ring but for one kernel -- the staged and mixed shapes at T = 6..8, which carry the most scalar state, among them.

Measured on the MI355X's host: the module takes 8.5 s on its own, 1.6 s of it the first test's set-up; its slowest test, staged
T = 8 over the delay ring, 0.6 s (eight calls, each with seven whole-table downloads of up to 12.6 MB), every other below 0.4 s.
The references are most of that time; a process that also runs tests/test_ntuple_update_matrix_cpu.py computes them once.

Tried once on scratch builds of the library (never committed; both touch a subset of the memory the correct kernels touch):
with dispatch_tuples sending T = 5 to the instantiation of T = 4, the nine tests of this module at T = 5 fail -- every family,
every source -- and no other (of tests/test_gpu_ntuple_play.py, the tests against the reference model at T = 5 fail; the
composition tests move with the shared dispatch, as the search matrix's do); with the three update bodies passing nullptr for
tc, so that a TC entry point reaches the TD kernel, all 69 tests of this module fail and no play test does.
"""
import numpy as np
import pytest

import ntuple_update_matrix as um
from analysis_helpers import g  # noqa: F401 (fixture)
from ntuple_tc_helpers import assert_tables_equal

pytestmark = pytest.mark.gpu
NAMES = ("weights", "err", "mag")


def device_case(g, torch, family, T, with_tc):
    """(NTupleNet, NTupleTC or None) of network T on the GPU: fresh copies, asserted to be the instantiation meant."""
    rnet, rtc = um.family_net(family, T)
    net, tc = um.device_state(g, torch, rnet, rtc if with_tc else None)
    assert net.n_tuples == T and (net.mixed, net.n_stages) == um.SHAPE[family]
    return net, tc


def check_one_call(g, torch, family, T, case, td_call, tc_call):
    """``td_call(net)`` and ``tc_call(net, tc, phases)`` launch the updates of a board or trace case."""
    base = um.base_tables(family, T)
    net, _ = device_case(g, torch, family, T, False)
    td_call(net)
    assert_tables_equal(um.tables(net), case.td.on(base[:1]), names=("td weights",))
    want = case.tc.on(base)
    for calls in ((3,), (1, 2)):
        net, tc = device_case(g, torch, family, T, True)
        for phases in calls:
            tc_call(net, tc, phases)
        assert_tables_equal(um.tables(net, tc), want, names=tuple(f"tc phases {calls}: {x}" for x in NAMES))


@pytest.mark.parametrize("case", um.CASES, ids=um.case_id)
def test_board_items(g, torch_cuda, case):
    torch = torch_cuda
    family, T = case
    um.assert_conditions(family, T, "board")
    c = um.board_case(family, T)
    boards, deltas = um.dev(torch, c.boards), um.dev(torch, c.deltas)
    check_one_call(g, torch, family, T, c, lambda net: net.update(boards, deltas, c.lr_shift),
                   lambda net, tc, phases: net.tc_update(boards, deltas, c.lr_shift, tc, phases))


@pytest.mark.parametrize("case", um.CASES, ids=um.case_id)
def test_trace_items(g, torch_cuda, case):
    torch = torch_cuda
    family, T = case
    um.assert_conditions(family, T, "trace")
    c = um.trace_case(family, T)
    tr = g.NTupleTrace(um.N, depth=um.H, lam=um.LAM / 65536)
    assert tr.lam_q16 == c.tr.lam
    tr.load_state_dict({"depth": um.H, "lam_q16": c.tr.lam, "slot": c.tr.slot, "hist": c.tr.hist, "len": c.tr.len})
    deltas = um.dev(torch, c.deltas)
    check_one_call(g, torch, family, T, c, lambda net: net.trace_update(tr, deltas, c.lr_shift),
                   lambda net, tc, phases: net.tc_trace_update(tr, deltas, c.lr_shift, tc, phases))
    assert tr.slot == c.tr.slot and np.array_equal(tr.hist.cpu().numpy(), c.tr.hist) and np.array_equal(tr.len.cpu().numpy(), c.tr.len)


@pytest.mark.parametrize("case", um.CASES, ids=um.case_id)
def test_delay_items(g, torch_cuda, case):
    """The ring and delta after every push, the tables after every update (TD; TC as one call; TC as two calls, each form on
    a network and accumulators of its own), and the ring unchanged by every update: ntuple_update_matrix.replay_delay."""
    family, T = case
    um.assert_conditions(family, T, "delay")
    td, tcs = um.replay_delay(g, torch_cuda, um.delay_case(family, T), splits=(um.ONE_CALL, um.TWO_CALLS))
    for net in [td] + [n for n, _ in tcs]:
        assert net.n_tuples == T and (net.mixed, net.n_stages) == um.SHAPE[family]
