"""CPU: the cases of tests/ntuple_update_matrix.py -- the 23 networks of the three families over board, trace and delay items --
through the host builds of the header's item code (tests/host_ntuple_mixed for board and trace items, always on
NtupleMixedShape; tests/host_ntuple_delay for the delay ring, on the family's own shape type), against the expected tables of
the pure-Python references, bit for bit and as whole arrays.  The expected values of tests/test_gpu_ntuple_update_matrix.py are
so checked twice without a GPU, pure Python against the C++ the kernels share: a failure that shows on the GPU alone points at
the instantiation, the launcher or the compiler, not at the test data.  Every test asserts ntuple_update_matrix.assert_conditions
first: what the inputs reach, from the references alone.

Measured on one core: the module takes 17 s on its own (4 s of it the g++ builds, when they are due), its slowest test, staged
T = 8 over the delay ring, 1.1 s; most of the rest is the references, which the GPU module shares when both run in one
process."""
import numpy as np
import pytest

import ntuple_delay_ref as dref
import ntuple_mixed_ref as mref
import ntuple_update_matrix as um
from ntuple_delay_helpers import host_push, host_update as host_delay_update, load_host_delay
from ntuple_mixed_helpers import host_trace_update, host_update, load_host_mixed
from ntuple_tc_helpers import assert_tables_equal

NAMES = ("weights", "err", "mag")


@pytest.fixture(scope="module")
def mixed_lib():
    return load_host_mixed()


@pytest.fixture(scope="module")
def delay_lib():
    return load_host_delay()


def state_of(family, T, flat):
    """(network, accumulators or None) holding the compact flat tables ``flat`` = (weights,) or (weights, err, mag)."""
    tuples, thr = um.family_tuples(family, T), um.family_thr(family)
    S = len(thr) + 1
    net = mref.mixed_net(tuples, thr, 10, flat[0].reshape(S, -1))
    return net, None if len(flat) == 1 else mref.tc_of(net, flat[1].reshape(S, -1), flat[2].reshape(S, -1))


def check_one_call(family, T, case, host):
    """``host(mode, net, tc)`` = (weights, err, mag) after the call: the TD update, the TC update with both phases, and each
    phase alone -- W writes the weights and leaves the accumulators, A the reverse."""
    base = um.base_tables(family, T)
    net, tc = um.family_net(family, T)
    want_td, want_tc = case.td.on(base[:1]), case.tc.on(base)
    assert_tables_equal(host(0, net, None)[:1], want_td, names=("td weights",))
    assert_tables_equal(host(3, net, tc), want_tc, names=tuple("tc " + x for x in NAMES))
    assert_tables_equal(host(1, net, tc), (want_tc[0], base[1], base[2]), names=tuple("phase W: " + x for x in NAMES))
    assert_tables_equal(host(2, net, tc), (base[0], want_tc[1], want_tc[2]), names=tuple("phase A: " + x for x in NAMES))
    assert_tables_equal(um.want_tables(net, tc), base)                              # (the host calls work on copies)


@pytest.mark.parametrize("case", um.CASES, ids=um.case_id)
def test_board_items(mixed_lib, case):
    family, T = case
    um.assert_conditions(family, T, "board")
    c = um.board_case(family, T)
    check_one_call(family, T, c, lambda mode, net, tc: host_update(mixed_lib, c.boards, c.deltas, c.lr_shift, mode, net, tc))


@pytest.mark.parametrize("case", um.CASES, ids=um.case_id)
def test_trace_items(mixed_lib, case):
    family, T = case
    um.assert_conditions(family, T, "trace")
    c = um.trace_case(family, T)
    check_one_call(family, T, c, lambda mode, net, tc: host_trace_update(mixed_lib, c.tr, c.deltas, c.lr_shift, mode, net, tc))


@pytest.mark.parametrize("case", um.CASES, ids=um.case_id)
def test_delay_items(delay_lib, case):
    """Every push and every update of the run from the reference's state before it, the items in another order from call to
    call: ascending, descending, stride 7."""
    family, T = case
    um.assert_conditions(family, T, "delay")
    run, kind = um.delay_case(family, T), um.KIND[family]
    base = um.base_tables(family, T)
    ring, td, tc = dref.Delay(run.n, run.depth, run.lam), base[:1], base
    for i, call in enumerate(run.calls):
        p, where = call.push, call.where
        if p is not None:
            got = host_push(delay_lib, ring, p.after, p.after_value, p.best_next, p.terminated)
            for name, a, b in zip(("hist", "len", "acc", "slot", "delta"), got, (call.ring.hist, call.ring.len, call.ring.acc_i64(), call.ring.slot, p.delta)):
                assert np.array_equal(a, b), f"{where}: {name}"
        ring, order = call.ring, i % 3
        want_td, want_tc = call.td.on(base[:1]), call.tc.on(base)
        net, _ = state_of(family, T, td)
        assert_tables_equal(host_delay_update(delay_lib, ring, run.lr_shift, 0, call.mode, order, net, kind)[:1], want_td, names=(f"{where}: td weights",))
        net, acc = state_of(family, T, tc)
        assert_tables_equal(host_delay_update(delay_lib, ring, run.lr_shift, 3, call.mode, order, net, kind, acc), want_tc,
                            names=tuple(f"{where}: tc {x}" for x in NAMES))
        assert_tables_equal(host_delay_update(delay_lib, ring, run.lr_shift, 1, call.mode, order, net, kind, acc), (want_tc[0], tc[1], tc[2]),
                            names=tuple(f"{where}: phase W: {x}" for x in NAMES))
        td, tc = want_td, want_tc
