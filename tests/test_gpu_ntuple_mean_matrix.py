"""GPU: every instantiation of the two batch-mean update kernels -- ntuple_mean_sum_kernel and ntuple_mean_apply_kernel over the
tuple counts T = 1..8, the three shape types and board and trace items -- against the pure-Python reference
(tests/ntuple_mean_ref.py on the padded array of ntuple_mixed_ref), bit for bit and as whole arrays: the weights after the call,
and sum and count all zero, once as one call with phases=3 and once as phases=1 then phases=2 on fresh copies (after phases=1 the
weights are untouched and sum and count are not zero).  There is no tolerance anywhere.

The networks, the 65-board pool, the ring (H = 4, 7 pushes) and the deltas are tests/ntuple_update_matrix.py's; the expected
tables are ntuple_mean_helpers.matrix_case's, which tests/test_ntuple_mean_host.py checks against the host build of the same item
code.  Every test first asserts ntuple_mean_helpers.assert_matrix_conditions -- from the reference and the inputs, never from
the device: the reference changes every one of the T tables in every one of the S stages (which fails for a launch of the
instantiation of T - 1, whose tables the test also builds and compares, and for a staged or mixed network sent to the uniform
shape); every table of every stage has an entry with a count of at least 2, so no table is only ever a plain update; entries
are reached by two items and twice by one; the weights differ from the summed update's.

Reached: 23 networks * 2 sources * 2 kernels = 92 of the 96 compiled kernels; not reached, as in
tests/test_gpu_ntuple_update_matrix.py, the mixed shape at T = 1, which the Python layer cannot select.
Fails on the parent commit: NTupleMean does not exist there."""
import numpy as np
import pytest

import ntuple_update_matrix as um
from analysis_helpers import g  # noqa: F401 (fixture)
from ntuple_mean_helpers import assert_matrix_conditions, assert_mean_tables, device_state, matrix_case, tables

pytestmark = pytest.mark.gpu


def device_case(g, torch, family, T):
    """(NTupleNet, NTupleMean) of network T on the GPU: fresh copies, asserted to be the instantiation meant."""
    net, mean = device_state(g, torch, um.family_net(family, T)[0])
    assert net.n_tuples == T and (net.mixed, net.n_stages) == um.SHAPE[family]
    return net, mean


def check_one_call(g, torch, family, T, c, call):
    """``call(net, mean, phases)`` launches the update of a board or trace case."""
    base = um.base_tables(family, T)[:1]
    want = c.want.on(base)[0]
    zero = np.zeros_like(want)
    for calls in ((3,), (1, 2)):
        net, mean = device_case(g, torch, family, T)
        for phases in calls:
            call(net, mean, phases)
            if phases == 1:
                w, s, n = tables(net, mean)
                assert np.array_equal(w, base[0]) and s.any() and n.any(), "phase SUM alone: the weights moved, or nothing was summed"
        assert_mean_tables(tables(net, mean), (want, zero, zero), f"phases {calls}: ")


@pytest.mark.parametrize("case", um.CASES, ids=um.case_id)
def test_board_items(g, torch_cuda, case):
    torch = torch_cuda
    family, T = case
    assert_matrix_conditions(family, T, "board")
    c = matrix_case(family, T, "board")
    boards, deltas = um.dev(torch, c.case.boards), um.dev(torch, c.case.deltas)
    check_one_call(g, torch, family, T, c, lambda net, mean, phases: net.mean_update(boards, deltas, c.case.lr_shift, mean, phases))


@pytest.mark.parametrize("case", um.CASES, ids=um.case_id)
def test_trace_items(g, torch_cuda, case):
    torch = torch_cuda
    family, T = case
    assert_matrix_conditions(family, T, "trace")
    c = matrix_case(family, T, "trace")
    ring = c.case.tr
    tr = g.NTupleTrace(um.N, depth=um.H, lam=um.LAM / 65536)
    assert tr.lam_q16 == ring.lam
    tr.load_state_dict({"depth": um.H, "lam_q16": ring.lam, "slot": ring.slot, "hist": ring.hist, "len": ring.len})
    deltas = um.dev(torch, c.case.deltas)
    check_one_call(g, torch, family, T, c, lambda net, mean, phases: net.mean_trace_update(tr, deltas, c.case.lr_shift, mean, phases))
    assert tr.slot == ring.slot and np.array_equal(tr.hist.cpu().numpy(), ring.hist) and np.array_equal(tr.len.cpu().numpy(), ring.len)
