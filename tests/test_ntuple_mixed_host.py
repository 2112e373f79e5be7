"""CPU: the mixed-length n-tuple code of g2048_device.h (NtupleMixedShape), compiled for the host
(tests/host_ntuple_mixed), against the reference tests/ntuple_mixed_ref.py -- the pure-Python references on a padded array --
bit for bit: the shape's lengths, bases and W, the element of every look-up, values, evaluate, search depth 1 and 2, the
TD(0) update, TC phases 1, 2 and 3, both trace updates, and S = 3 staged.  Weights are full-range random int32 over the
whole compact array, so a look-up one element off, or in a neighbour's table, reads another number.  Every test shows from
the reference's look-up trace (never from the code under test) that it reaches the edge it names."""
import numpy as np
import pytest

import ntuple_mixed_ref as mref
import ntuple_ref as ref
import ntuple_staged_ref as sref
import ntuple_trace_ref as tref
from ntuple_helpers import TUPLES_17x4, assert_eval_equal
from ntuple_mixed_helpers import (THR_3, boards_67, deep, host_evaluate, host_offsets, host_search, host_shape, host_trace_update,
                                  host_update, host_values, load_host_mixed, near_full_12, net_of, pushed_trace, random_tc, shallow,
                                  staged_boards, want_tables)
from ntuple_search_helpers import assert_search_equal
from ntuple_staged_helpers import small_boards
from ntuple_tc_helpers import assert_tables_equal, edge_deltas
from ntuple_trace_helpers import push_inputs, trace_deltas

@pytest.fixture(scope="module")
def lib():
    return load_host_mixed()


# ------------------------------------------------------------------------------------------------ layout
def test_compact_and_expand_follow_the_definition():
    assert mref.lens(mref.MIX_ASC) == [1, 2, 3, 4] and mref.bases(mref.MIX_ASC) == [0, 16, 272, 4368]
    assert mref.n_weights(mref.MIX_ASC) == 69904 and mref.n_weights(mref.PRESET) == 4 * 16 ** 6 + 4 * 16 ** 4 == 67371008
    assert mref.lens(mref.MIX_8) == [4, 1, 3, 2, 4, 2, 3, 1] and len(mref.MIX_8) == 8
    flat = np.arange(2 * 69904).reshape(2, 69904)
    padded = mref.expand(flat, mref.MIX_ASC)
    assert padded.shape == (2, 4, 16 ** 4) and padded[1, 2, 5] == 69904 + 272 + 5 and padded[0, 0, 16] == 0
    assert np.array_equal(mref.compact(padded, mref.MIX_ASC), flat)
    assert np.array_equal(mref.compact(mref.expand(flat[0], mref.MIX_ASC), mref.MIX_ASC), flat[0])


@pytest.mark.parametrize("name", sorted(mref.SHAPES))
def test_shape_and_every_look_up_offset(lib, name):
    net, boards = net_of(name), boards_67()
    tuples = net.tuples
    assert host_shape(lib, net) == (1, mref.n_weights(tuples), mref.lens(tuples), mref.bases(tuples))
    assert all(b % 4 == 0 for b in mref.bases(tuples))                      # every table starts 16-byte aligned
    want = np.array([sorted(mref.lookups(b, net)) for b in boards])
    got = np.sort(host_offsets(lib, boards, net).astype(np.int64), axis=1)
    assert got.max() < mref.n_weights(tuples) and np.array_equal(got, want)
    # tuple_len above the longest list: more END entries, the same network
    if max(mref.lens(tuples)) < 6:
        assert host_shape(lib, net, 6) == host_shape(lib, net)
        assert np.array_equal(np.sort(host_offsets(lib, boards, net, 6).astype(np.int64), axis=1), want)


def test_shape_of_an_end_free_descriptor_is_not_mixed(lib):
    net = mref.mixed_net(TUPLES_17x4)
    assert host_shape(lib, net) == (0, 5 * 16 ** 4, [4] * 5, [t * 16 ** 4 for t in range(5)])
    assert host_shape(lib, net, 6)[0] == 1                                  # the equal cut: END-padded, the same layout
    assert host_shape(lib, net, 6)[1:] == host_shape(lib, net)[1:]


# ------------------------------------------------------------------------------------------------ values, evaluate, search
@pytest.mark.parametrize("name", sorted(mref.SHAPES))
def test_values_evaluate_search_depth_1(lib, name):
    net, boards = net_of(name), boards_67()
    assert mref.table_edges(boards, net) == mref.all_edges(net)             # first and last entry of each table are read
    want_v, want_e, want_s = shallow(name)
    assert np.array_equal(host_values(lib, boards, net), want_v)
    assert want_v[64] == 8 * sum(int(mref.flat_of(net)[0, b]) for b in mref.bases(net.tuples))             # [0]*16: entry 0
    assert want_v[65] == want_v[66] == 8 * sum(int(mref.flat_of(net)[0, b + 16 ** n - 1])
                                               for b, n in zip(mref.bases(net.tuples), mref.lens(net.tuples)))
    q = want_e[0]
    assert len(set(q[60].tolist())) == 1 and q[60, 0] != ref.ILLEGAL and want_e[1][60] == 0               # the tie
    assert (q[62] != ref.ILLEGAL).sum() == 1 and (q[63] == ref.ILLEGAL).all()
    assert_eval_equal(host_evaluate(lib, boards, net), want_e, boards, "evaluate")
    assert len(set(want_s[0].tolist())) == 4
    assert_search_equal(host_search(lib, boards, 1, net), want_s, boards, "search depth 1")


@pytest.mark.parametrize("name", sorted(mref.SHAPES))
def test_search_depth_2(lib, name):
    net, boards = net_of(name), near_full_12()
    assert ((boards == 0).sum(1) <= 2).all()
    want = deep(name)
    assert (want[1][-1] == ref.ILLEGAL).all() and (want[1][:-1] != ref.ILLEGAL).any(1).all()
    assert_search_equal(host_search(lib, boards, 2, net), want, boards, "search depth 2")


# ------------------------------------------------------------------------------------------------ updates
@pytest.mark.parametrize("name", sorted(mref.SHAPES))
def test_update_and_tc_phases(lib, name):
    net, boards = net_of(name), boards_67()
    deltas = edge_deltas(len(boards), 93)
    deltas[64:] = (5 << 20, -7 << 20, 3 << 20)                              # the edge boards take a step
    want = net.copy()
    sref.update(want, boards, deltas, 3)
    assert (mref.flat_of(want) != mref.flat_of(net)).any()
    assert_tables_equal(host_update(lib, boards, deltas, 3, 0, net)[:1], want_tables(want))
    tc = random_tc(net, 94)
    for phases in (1, 2, 3):
        wn, wt, trace = net.copy(), tc.copy(), {}
        sref.tc_update(wn, wt, boards, deltas, 2, phases, trace)
        assert trace["stage"] == {0: len(boards)}
        assert_tables_equal(host_update(lib, boards, deltas, 2, phases, net, tc), want_tables(wn, wt))
        assert (mref.flat_of(wn) != mref.flat_of(net)).any() == bool(phases & 1) and (wt.err != tc.err).any() == bool(phases & 2)


@pytest.mark.parametrize("name", sorted(mref.SHAPES))
def test_trace_updates(lib, name):
    net, n = net_of(name), 24
    tr = pushed_trace(n, 3, 40000, 95)
    deltas = trace_deltas(n, 96)
    deltas[:3] = (5 << 20, -7 << 20, 3 << 20)
    live = tr.hist[tr.slot, :3]
    assert mref.table_edges(live, net) == mref.all_edges(net)
    want, trace = net.copy(), {}
    sref.trace_update(want, tr, deltas, 3, trace)
    assert trace["hist_span"] == 0 and (mref.flat_of(want) != mref.flat_of(net)).any()
    assert_tables_equal(host_trace_update(lib, tr, deltas, 3, 0, net)[:1], want_tables(want))
    tc = random_tc(net, 97)
    wn, wt = net.copy(), tc.copy()
    sref.tc_trace_update(wn, wt, tr, deltas, 2, 3)
    assert_tables_equal(host_trace_update(lib, tr, deltas, 2, 3, net, tc), want_tables(wn, wt))


# ------------------------------------------------------------------------------------------------ staged, S = 3
def test_staged_values_evaluate_search(lib):
    net, boards = net_of("asc", THR_3), staged_boards()
    trace = {}
    want_v = sref.values_batch(boards, net, trace)
    assert set(trace["stage"]) == {0, 1, 2}                                       # all S stages are read
    for s in range(3):                                                       # ... and the table edges within the weight sets
        part = boards[sref.stage_batch(boards, net.thr) == s]
        assert len(part) > 0
    assert sref.stage_batch(boards[-3:], net.thr).tolist() == [0, 2, 2]
    W = mref.n_weights(net.tuples)
    got_off = host_offsets(lib, boards, net).astype(np.int64)
    assert np.array_equal(np.sort(got_off, axis=1), np.array([sorted(mref.lookups(b, net)) for b in boards]))
    assert got_off.max() < 3 * W and (got_off // W == sref.stage_batch(boards, net.thr)[:, None]).all()
    assert got_off[-3].min() == 0 and got_off[-1].max() == 3 * W - 1        # the first and the last element of the array
    assert np.array_equal(host_values(lib, boards, net), want_v)
    trace = {}
    want_e = sref.evaluate_batch(boards, net, trace)
    assert trace["after_span"] > 0                                           # afterstates in a stage other than their board's
    assert_eval_equal(host_evaluate(lib, boards, net), want_e, boards, "staged evaluate")
    trace = {}
    want_s = sref.search_batch(boards, 1, net, trace)
    assert trace["leaf_other"] > 0 and trace["chance_span"] > 0
    assert_search_equal(host_search(lib, boards, 1, net), want_s, boards, "staged search depth 1")
    deep = np.concatenate([boards[np.argsort((boards == 0).sum(1), kind="stable")[:6]], near_full_12()[:4]])
    trace = {"memo": {}}
    want_d = sref.search_batch(deep, 2, net, trace)
    assert trace["leaf_other"] > 0
    assert_search_equal(host_search(lib, deep, 2, net), want_d, deep, "staged search depth 2")


def test_staged_updates(lib):
    net, boards = net_of("asc", THR_3), staged_boards()
    deltas = edge_deltas(len(boards), 98)
    deltas[-3:] = (5 << 20, -7 << 20, 3 << 20)
    want, trace = net.copy(), {}
    sref.update(want, boards, deltas, 3, trace)
    assert set(trace["stage"]) == {0, 1, 2}
    changed = (mref.flat_of(want) != mref.flat_of(net)).any(1)
    assert changed.all()                                                     # every weight set is written
    assert_tables_equal(host_update(lib, boards, deltas, 3, 0, net)[:1], want_tables(want))
    tc = random_tc(net, 99)
    for phases in (1, 2, 3):
        wn, wt = net.copy(), tc.copy()
        sref.tc_update(wn, wt, boards, deltas, 2, phases)
        assert_tables_equal(host_update(lib, boards, deltas, 2, phases, net, tc), want_tables(wn, wt))
    n = 24
    tr = tref.Trace(n, 3, 40000)
    pool = small_boards(n * 5, 100).reshape(5, n, 16)
    for t, (_, av, best, term) in enumerate(push_inputs(n, 5, 101)):
        tref.push(tr, pool[t], av, best, term)
    td = trace_deltas(n, 102)
    wn, wt, trace = net.copy(), tc.copy(), {}
    sref.tc_trace_update(wn, wt, tr, td, 2, 3, trace)
    assert trace["hist_span"] > 0 and set(trace["stage"]) == {0, 1, 2}      # one board's slots in different stages
    assert_tables_equal(host_trace_update(lib, tr, td, 2, 3, net, tc), want_tables(wn, wt))
    wn = net.copy()
    sref.trace_update(wn, tr, td, 3)
    assert_tables_equal(host_trace_update(lib, tr, td, 3, 0, net)[:1], want_tables(wn))
