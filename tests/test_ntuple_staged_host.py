"""CPU: the multi-stage n-tuple code of g2048_device.h compiled for the host (tests/host_ntuple/ntuple_check.cpp)
equals the pure-Python reference (tests/ntuple_staged_ref.py) bit for bit -- mask, stage, evaluate, values, the TD(0), TC and
trace updates and the depth-1..2 search -- S = 1 equals the unstaged host build, the library refuses a bad staged
descriptor before it touches a device, and the Python layer checks ``stages=``, ``stage_mask`` and ``promote``.  Every test
shows from the reference's trace (never from the code under test) that its input reaches the edge it names."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
import ntuple_ref as ref
import ntuple_staged_ref as sref
import ntuple_trace_ref as tref
from ntuple_helpers import (TUPLES_17x4, TUPLES_8x4, assert_eval_equal, host_base, host_evaluate, host_mask, host_search, host_stage,
                            host_trace_update, host_update, host_values, load_host_ntuple)
from ntuple_staged_helpers import (LOW_THR, THR_8, preload_tc, small_boards, with_deficit_bits, depth2_boards, sparse_boards,
                                   ONE_TUPLE)
from ntuple_tc_helpers import assert_tables_equal
from ntuple_trace_helpers import trace_deltas

N = 100


@pytest.fixture(scope="module")
def hl():
    return load_host_ntuple()


@pytest.fixture(scope="module")
def boards():
    return small_boards(N, 5)


@pytest.fixture(scope="module")
def net():
    return sref.random_net(TUPLES_17x4, LOW_THR, 21, lo=-(1 << 30), hi=1 << 30)


def test_mask_of_every_exponent_and_of_engine_records(hl):
    """Every single-tile exponent 0..31 on an otherwise empty board (the cap at 15: exponents 15..31 share bit 15), bytes
    above 31 (taken mod 32), and the engine-record form with score-deficit bits set."""
    single = np.zeros((32, 16), np.uint8)
    single[np.arange(32), np.arange(32) % 16] = np.arange(32)
    want = [1 | (1 << min(e, 15)) for e in range(32)]
    assert [sref.mask(b) for b in single] == want and host_mask(hl, single).tolist() == want
    assert sref.mask([0] * 16) == 1 and sref.mask(list(range(16))) == 0xffff and sref.mask([3] * 16) == 8
    assert host_mask(hl, np.array([[0] * 16, list(range(16)), [3] * 16], np.uint8)).tolist() == [1, 0xffff, 8]
    plain = small_boards(64, 6, max_exp=31)
    want = [sref.mask(ref.plain(b)) for b in plain]
    assert len({m >> 15 for m in want}) == 2
    assert host_mask(hl, plain).tolist() == want
    raw = with_deficit_bits(plain, 7)
    assert (raw[:, 8:] > 31).any() and host_mask(hl, raw).tolist() == want
    assert host_mask(hl, plain | 0xe0).tolist() == want          # exponents mod 32


@pytest.mark.parametrize("S", [1, 2, 8])
def test_stage_at_above_and_below_a_threshold(hl, S):
    """Thresholds equal to a board's mask, one above and one below it; S in {1, 2, 8}."""
    plain = small_boards(N, 8)
    masks = sorted({sref.mask(ref.plain(b)) for b in plain})
    assert len(masks) >= 8
    for shift in (0, 1, -1):
        picks = masks[len(masks) // 2:][:S - 1] if S == 2 else masks[1:S]
        thr = tuple(m + shift for m in picks)
        snet, trace = sref.StagedNet(TUPLES_17x4, thr), {}
        want = sref.stage_batch(plain, thr, trace)
        if S > 1:                                       # a mask at, one below, one above a threshold
            assert trace["at_thr"] > 0 if shift == 0 else trace["below_thr"] > 0 if shift == 1 else any(m - 1 in thr for m in masks)
        assert S == 1 or len(trace["stage"]) >= 2
        assert host_stage(hl, plain, snet).tolist() == want.tolist()
        assert host_stage(hl, with_deficit_bits(plain, 9), snet).tolist() == want.tolist()
        assert host_base(hl, plain, snet).tolist() == (want.astype(np.int64) * 5 * 16 ** 4).tolist()
    full = sref.StagedNet(TUPLES_17x4, THR_8)
    trace = {}
    want = sref.stage_batch(plain, THR_8, trace)
    assert sorted(trace["stage"]) == list(range(8)) or S != 8
    assert host_stage(hl, plain, full).tolist() == want.tolist()
    # the extremes: threshold 1 is reached by the lowest mask there is, 65535 only by the board of 16 different cells
    ends = sref.StagedNet(TUPLES_17x4, (1, 65535))
    edge = np.array([[1] * 16, [0] * 16, list(range(16))], np.uint8)
    assert host_stage(hl, edge, ends).tolist() == sref.stage_batch(edge, ends.thr).tolist() == [1, 1, 2]


def test_evaluate_and_values(hl, boards, net):
    trace = {}
    want = sref.evaluate_batch(boards, net, trace)
    assert sorted(trace["stage"]) == [0, 1, 2, 3] and trace["after_span"] >= 5
    assert_eval_equal(host_evaluate(hl, boards, net), want, boards, "staged evaluate")
    vtrace = {}
    assert np.array_equal(host_values(hl, boards, net), sref.values_batch(boards, net, vtrace))
    assert sorted(vtrace["stage"]) == [0, 1, 2, 3]


@pytest.mark.parametrize("depth", [1, 2])
def test_search(hl, boards, net, depth):
    """A spawned 4 crosses stage_mask(4): chance nodes whose children lie in two stages, leaves in another stage than the
    root."""
    sub = boards if depth == 1 else depth2_boards(boards)
    trace = {}
    act, val = sref.search_batch(sub, depth, net, trace)
    assert trace["chance_span"] > 0 and trace["leaf_other"] > 0 and len(trace["stage"]) == 4
    got_act, got_val = host_search(hl, sub, depth, net)
    assert np.array_equal(got_val, val) and np.array_equal(got_act, act)


def test_search_depth_2_on_sparse_boards(hl):
    """24 boards with 5..8 empty cells under a one-tuple network with S = 4: wide chance nodes, which the few full boards of
    test_search do not have."""
    sub = sparse_boards(24, 91)
    one = sref.random_net(ONE_TUPLE, LOW_THR, 92, lo=-(1 << 30), hi=1 << 30)
    trace = {"memo": {}}
    act, val = sref.search_batch(sub, 2, one, trace)
    assert ((sub == 0).sum(1) >= 5).all() and trace["leaf_other"] > 0 and len(trace["stage"]) >= 3
    assert len(set(sref.stage_batch(sub, LOW_THR).tolist())) == 4
    got_act, got_val = host_search(hl, sub, 2, one)
    assert np.array_equal(got_val, val) and np.array_equal(got_act, act)


def test_updates(hl, boards, net):
    deltas = trace_deltas(N, 31)
    trace = {}
    want = net.copy()
    sref.update(want, boards, deltas, 3, trace)
    assert sorted(trace["stage"]) == [0, 1, 2, 3]
    assert_tables_equal((host_update(hl, boards, deltas, 3, 0, net)[0],), (want.weights,))
    tc = preload_tc(net, 32)
    for phases in (3, 1, 2):
        want, want_tc = net.copy(), tc.copy()
        sref.tc_update(want, want_tc, boards, deltas, 2, phases)
        assert_tables_equal(host_update(hl, boards, deltas, 2, phases, net, tc), (want.weights, want_tc.err, want_tc.mag_i64()))


@pytest.mark.parametrize("H", [1, 8])
def test_trace_updates(hl, net, H):
    n = 40
    tr = tref.Trace(n, H, 49152)
    for p in range(H + 2):
        tref.push(tr, small_boards(n, 40 + p), np.zeros(n, np.int64), np.zeros(n, np.int64), (np.arange(n) + p) % 7 == 0)
    deltas = trace_deltas(n, 33)
    trace = {}
    want = net.copy()
    sref.trace_update(want, tr, deltas, 1, trace)
    assert len(trace["stage"]) == 4 and (trace["hist_span"] > 0) == (H > 1)
    assert_tables_equal((host_trace_update(hl, tr, deltas, 1, 0, net)[0],), (want.weights,))
    tc = preload_tc(net, 34)
    want, want_tc = net.copy(), tc.copy()
    sref.tc_trace_update(want, want_tc, tr, deltas, 2, 3)
    assert_tables_equal(host_trace_update(hl, tr, deltas, 2, 3, net, tc), (want.weights, want_tc.err, want_tc.mag_i64()))


def test_one_stage_is_the_unstaged_network(hl, boards):
    """S = 1: the same bits as the unstaged host build and the unstaged reference."""
    one = sref.random_net(TUPLES_8x4[:6], (), 41)
    plain = ref.Net(one.tuples, one.frac_bits, one.weights[0])
    assert_eval_equal(host_evaluate(hl, boards, one), host_evaluate(hl, boards, plain), boards, "S = 1")
    assert_eval_equal(host_evaluate(hl, boards, one), ref.evaluate_batch(boards, plain), boards, "S = 1 vs reference")
    assert np.array_equal(host_values(hl, boards, one), host_values(hl, boards, plain))
    deltas = trace_deltas(N, 42)
    assert np.array_equal(host_update(hl, boards, deltas, 2, 0, one)[0][0], host_update(hl, boards, deltas, 2, 0, plain)[0])
    assert not host_base(hl, boards, one).any()


# ------------------------------------------------------------------------------------------------ the library and Python
@pytest.fixture(scope="module")
def lib():
    ge.build_hip()
    from gym2048_amd import _lib
    return _lib.load()


BOARDS, OUT, WEIGHTS = 0x10000, 0x20000, 0x30000      # fake device addresses: every call below is refused before they are used


def _staged(S, thr, weights=WEIGHTS):
    from gym2048_amd import _lib
    net = _lib.NTupleStagedNetC(_lib.NTupleNetC(5, 4, 10), S)
    for t, cells in enumerate(TUPLES_17x4):
        for k, c in enumerate(cells):
            net.net.cells[t][k] = c
    net.net.weights = weights
    net.thresholds[:len(thr)] = thr
    return net


def _calls(lib, ref_):
    from gym2048_amd import _lib
    io, sio = _lib.NTupleIO(action=OUT), _lib.NTupleSearchIO(1, OUT, None)
    tc, tr = _lib.NTupleTCC(OUT, OUT), _lib.NTupleTraceC(4, 32768, OUT, OUT)
    return (lambda: lib.g2048_ntuple_staged_evaluate_plain(BOARDS, 4, ref_, C.byref(io), None),
            lambda: lib.g2048_ntuple_staged_search_plain(BOARDS, 4, ref_, C.byref(sio), None),
            lambda: lib.g2048_ntuple_staged_values_plain(BOARDS, 4, ref_, OUT, None),
            lambda: lib.g2048_ntuple_staged_update_plain(BOARDS, 4, OUT, 3, ref_, None),
            lambda: lib.g2048_ntuple_staged_tc_update_plain(BOARDS, 4, OUT, 3, 3, ref_, C.byref(tc), None),
            lambda: lib.g2048_ntuple_staged_trace_update(4, OUT, 3, ref_, C.byref(tr), 0, None),
            lambda: lib.g2048_ntuple_staged_tc_trace_update(4, OUT, 3, 3, ref_, C.byref(tc), C.byref(tr), 0, None),
            lambda: lib.g2048_ntuple_stage_plain(BOARDS, 4, ref_, OUT, None))


STAGED_ERRORS = [
    (lambda: _staged(3, (8, 4)), b"thresholds[1]=4: thresholds must be strictly ascending"),
    (lambda: _staged(3, (4, 4)), b"thresholds[1]=4: thresholds must be strictly ascending"),
    (lambda: _staged(3, (0, 4)), b"thresholds[0]=0"),
    (lambda: _staged(2, (0,)), b"thresholds[0]=0"),
    (lambda: _staged(0, ()), b"n_stages=0"),
    (lambda: _staged(9, (1, 2, 3, 4, 5, 6, 7)), b"n_stages=9"),
    (lambda: None, b"net is NULL"),
]


@pytest.mark.parametrize("make, message", STAGED_ERRORS, ids=["descending", "equal", "zero", "zero-only", "S=0", "S=9", "NULL"])
def test_bad_staged_descriptor_in_every_entry_point(lib, make, message):
    net = make()
    for call in _calls(lib, None if net is None else C.byref(net)):
        assert call() == -1
        assert message in lib.g2048_last_error()


def test_staged_descriptor_layout_and_inner_network_errors(lib):
    from gym2048_amd import _lib
    S = _lib.NTupleStagedNetC
    assert (C.sizeof(S), S.net.offset, S.n_stages.offset, S.thresholds.offset) == (96, 0, 72, 76)
    assert "#define G2048_NTUPLE_MAX_STAGES 8\n" in open(ge.ROOT + "/include/g2048.h").read()
    # thresholds past S - 1 are ignored; the inner network is checked as the unstaged calls check it
    ok = _staged(2, (4, 0, 9, 3))
    assert lib.g2048_ntuple_staged_values_plain(BOARDS, 4, C.byref(ok), None, None) == -1 and b"v is NULL" in lib.g2048_last_error()
    bad = _staged(2, (4,), weights=None)
    for call in _calls(lib, C.byref(bad))[:-1]:
        assert call() == -1 and b"net weights is NULL" in lib.g2048_last_error()
    # the stage-only call reads no weights
    assert lib.g2048_ntuple_stage_plain(BOARDS, 4, C.byref(bad), None, None) == -1 and b"stage is NULL" in lib.g2048_last_error()
    bad.net.n_tuples = 9
    assert lib.g2048_ntuple_stage_plain(BOARDS, 4, C.byref(bad), OUT, None) == -1 and b"n_tuples=9" in lib.g2048_last_error()


def test_python_layer_checks_its_input():
    torch = pytest.importorskip("torch")
    from gym2048_amd import ntuple
    assert ntuple.stage_mask(16384, 8192) == 0x6000 and ntuple.stage_mask(16384) == 0x4000 and ntuple.stage_mask(32768) == 0x8000
    assert ntuple.stage_mask(32768, 16384) == 0xC000 and ntuple.stage_mask(2) == 2 and ntuple.stage_mask(65536) == 0x8000
    assert ntuple.stage_mask(4) == sref.stage_mask(4) and ntuple.stage_mask(16, 8) == sref.stage_mask(16, 8) == 24
    for bad in ((), (3,), (1,), (0,), (2.0,), (True,)):
        with pytest.raises(ValueError, match="tile"):
            ntuple.stage_mask(*bad)
    for bad in ((8, 4), (4, 4), (0,), (65536,), (1.5,), range(1, 9), 5):
        with pytest.raises(ValueError, match="stages"):
            ntuple.NTupleNet("17x4", device="cpu", stages=bad)
    net = ntuple.NTupleNet("17x4", frac_bits=12, device="cpu", stages=LOW_THR)
    assert tuple(net.weights.shape) == (4, 5, 16 ** 4) and net.stages == LOW_THR and net.n_stages == 4
    assert (net._c.n_stages, list(net._c.thresholds)[:3], net._c.net.weights) == (4, list(LOW_THR), net.weights.data_ptr())
    assert [net._c.net.cells[3][k] for k in range(4)] == [1, 2, 5, 6] and net._fn("values_plain").__name__ == "g2048_ntuple_staged_values_plain"
    one = ntuple.NTupleNet("17x4", device="cpu", stages=())
    assert tuple(one.weights.shape) == (1, 5, 16 ** 4) and one.n_stages == 1
    plain = ntuple.NTupleNet("17x4", frac_bits=12, device="cpu")
    assert plain.stages is None and tuple(plain.weights.shape) == (5, 16 ** 4) and plain._fn("values_plain").__name__ == "g2048_ntuple_values_plain"
    tc = ntuple.NTupleTC(net)
    assert tc.err.shape == tc.mag.shape == net.weights.shape and "S times" in ntuple.NTupleTC.__doc__
    # promote
    for call in (lambda: plain.promote(0, 1), lambda: plain.stage(torch.zeros((4, 16), dtype=torch.uint8))):
        with pytest.raises(ValueError, match="staged network"):
            call()
    for bad in ((1, 1), (0, 4), (-1, 0), (0, 1.0)):
        with pytest.raises(ValueError, match="src|dst"):
            net.promote(*bad)
    with pytest.raises(ValueError, match="tc must be"):
        net.promote(0, 1, ntuple.NTupleTC(plain))
    with pytest.raises(ValueError, match="boards"):
        net.stage(torch.zeros((4, 16), dtype=torch.uint8))     # host tensor
    net.weights[1, 2, 77], net.weights[3, 0, 5] = -5, 9
    tc.err[2, 2, 77], tc.mag[2, 2, 77], tc.err[1, 0, 0] = 3, 4, 6
    net.promote(1, 2, tc)
    assert net.weights[2, 2, 77] == -5 and net.weights[3, 0, 5] == 9 and int(net.weights.count_nonzero()) == 3
    assert not tc.err[2].any() and not tc.mag[2].any() and tc.err[1, 0, 0] == 6
    # state_dict carries the stages; loading across different stages raises
    other = ntuple.NTupleNet("17x4", frac_bits=12, device="cpu", stages=LOW_THR)
    other.load_state_dict(net.state_dict())
    assert torch.equal(other.weights, net.weights) and net.state_dict()["stages"] == LOW_THR
    for wrong in (plain, ntuple.NTupleNet("17x4", frac_bits=12, device="cpu", stages=(4, 8, 25))):
        with pytest.raises(ValueError, match="stages"):
            wrong.load_state_dict(net.state_dict())
        with pytest.raises(ValueError, match="stages"):
            net.load_state_dict(wrong.state_dict())
    legacy = {k: v for k, v in plain.state_dict().items() if k != "stages"}
    plain.load_state_dict(legacy)                               # a state saved before stages existed is an unstaged one
