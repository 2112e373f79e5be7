"""CPU: the n-tuple delay of g2048_device.h compiled for the host (tests/host_ntuple_delay/delay_check.cpp: the header's push
function and the item loop over NtupleDelayItems, wrapping adds for the atomic ones) against tests/ntuple_delay_ref.py, bit
for bit: hist, len, acc and delta after every push; the tables after the TD update, TC phase W and TC phase A of every push
(STEP) and after the FLUSH -- with the items visited in ascending, descending and stride-7 order, which must give the same
tables: the result does not depend on the launch geometry.  T = 1, 4 and 8, one staged and one mixed network."""
import numpy as np
import pytest

import ntuple_delay_ref as dref
import ntuple_mixed_ref as mref
from ntuple_delay_helpers import ORDERS, host_push, host_update, load_host_delay
from ntuple_helpers import TUPLES_8x4
from ntuple_mixed_helpers import THR_3, random_tc, want_tables
from ntuple_staged_helpers import small_boards
from ntuple_tc_helpers import assert_tables_equal
from ntuple_trace_helpers import push_inputs


@pytest.fixture(scope="module")
def lib():
    return load_host_delay()


def test_due_over_every_len_byte(lib):
    for H in range(1, 9):
        for b in range(256):
            for k in range(9):
                for mode in (0, 1):
                    assert lib.delay_check_due(b, k, H, mode) == int(bool(dref.is_due(b, k, H, mode))), (H, b, k, mode)


@pytest.mark.parametrize("H", range(1, 9))
def test_push_over_every_len_byte(lib, H):
    """Every old byte, both flags, accumulators near +-2^43: the host push writes the reference's len, acc and delta."""
    rng = np.random.default_rng(60 + H)
    for term in (0, 1):
        dl = dref.Delay(256, H, 50000)
        dl.len[:] = np.arange(256, dtype=np.uint8)
        dl.slot = H // 2
        dl.acc = [[int(x) for x in rng.integers(-(7 << 40), 7 << 40, 256)] for _ in range(H)]
        after = rng.integers(0, 18, (256, 16)).astype(np.uint8)
        av, best = rng.integers(-(1 << 62), 1 << 62, 256), rng.integers(-(1 << 62), 1 << 62, 256)
        av[:6], best[:6] = 0, [1 << 40, -(1 << 40), (1 << 40) + 1, -(1 << 40) - 1, (1 << 63) - 1, -(1 << 63)]
        got = host_push(lib, dl, after, av, best, np.full(256, term * 0xff, np.uint8))
        delta = dref.push(dl, after, av, best, np.full(256, term))
        for name, g, w in zip(("hist", "len", "acc", "slot", "delta"), got, (dl.hist, dl.len, dl.acc_i64(), dl.slot, delta)):
            assert np.array_equal(g, w), (name, H, term)


CASES = {
    "T=1": (TUPLES_8x4[:1], (), 0, 4, 40000), "T=4": (TUPLES_8x4[:4], (), 0, 1, 32768), "T=8": (TUPLES_8x4, (), 0, 8, 65536),
    "staged T=3 S=3": (TUPLES_8x4[:3], THR_3, 1, 3, 40000), "mixed T=4": (mref.MIX_ASC, (), 2, 4, 20000),
    "mixed staged": (mref.MIX_DESC, THR_3, 2, 2, 65535),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_pushes_updates_and_flush_in_three_item_orders(lib, name):
    tuples, thr, kind, H, lam = CASES[name]
    n, pushes = 24, H + 4
    S = len(thr) + 1
    net = mref.mixed_net(tuples, thr, 10, mref.random_flat(tuples, 70, S))
    td, tcn, tc = net.copy(), net.copy(), random_tc(net, 71)
    dl = dref.Delay(n, H, lam)
    pool = small_boards(n * pushes, 72).reshape(pushes, n, 16)      # small boards: THR_3 puts them into every stage
    applied = {dref.STEP: 0, dref.FLUSH: 0}

    def updates(mode):
        boards, Ds = dref.due_items(dl, mode)
        applied[mode] += len(Ds)
        for form, (wn, wt) in ((0, (td, None)), (1, (tcn, tc)), (2, (tcn, tc))):
            got = [host_update(lib, dl, 2, form, mode, o, wn, kind, wt) for o in ORDERS.values()]
            if form == 0:
                dref.delay_update(wn, dl, 2, mode)
            else:
                dref.tc_delay_update(wn, wt, dl, 2, form, mode)
            want = want_tables(wn, wt)
            for order, g in zip(ORDERS, got):
                assert_tables_equal(g[:len(want)], want, names=tuple(f"{name} form {form} mode {mode} {order}: {x}" for x in ("weights", "err", "mag")))

    for t, (_, av, best, term) in enumerate(push_inputs(n, pushes, 73)):
        got = host_push(lib, dl, pool[t], av, best, term)
        delta = dref.push(dl, pool[t], av, best, term)
        for what, g, w in zip(("hist", "len", "acc", "slot", "delta"), got, (dl.hist, dl.len, dl.acc_i64(), dl.slot, delta)):
            assert np.array_equal(g, w), (what, t)
        updates(dref.STEP)
    assert (mref.flat_of(td) != mref.flat_of(net)).any() and (mref.flat_of(tcn) != mref.flat_of(net)).any()
    if H > 1:
        assert len(dref.due_items(dl, dref.FLUSH)[1]) > 0
    updates(dref.FLUSH)
    assert applied[dref.STEP] + applied[dref.FLUSH] == n * pushes      # every pushed afterstate exactly once
    if S > 1:
        assert (mref.flat_of(td) != mref.flat_of(net)).any(1).all()     # every weight set is written
