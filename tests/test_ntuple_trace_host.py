"""CPU: the n-tuple trace code of g2048_device.h -- the header the kernels are compiled from -- built for the host
(tests/host_ntuple/ntuple_check.cpp, g++) and compared bit for bit with the pure-Python reference
tests/ntuple_trace_ref.py.  Every test shows from the reference's own trace (never from the code under test) that its input
reaches the edge it names."""
import numpy as np
import pytest

import ntuple_ref as ref
import ntuple_tc_ref as tcref
import ntuple_trace_ref as tref
from analysis_helpers import mixed_boards
from ntuple_helpers import TUPLES_17x4, host_push, host_trace_update, host_update, load_host_ntuple, random_net, raw_desc
from ntuple_tc_helpers import assert_tables_equal, preload
from ntuple_trace_helpers import INT64_MAX, INT64_MIN, push_inputs, trace_deltas

LAMS = (0, 1, 32768, 65535, 65536)


@pytest.fixture(scope="module")
def ht():
    return load_host_ntuple()


def filled(n, H, lam, pushes, seed, trace=None, lib=None):
    """A reference trace after ``pushes`` synthetic pushes (checked against the host build push by push when ``lib``)."""
    tr = tref.Trace(n, H, lam)
    for after, av, bn, term in push_inputs(n, pushes, seed):
        if lib is not None:
            got, got_delta = host_push(lib, tr, after, av, bn, term)
        delta = tref.push(tr, after, av, bn, term, trace)
        if lib is not None:
            assert got.slot == tr.slot and np.array_equal(got.hist, tr.hist) and np.array_equal(got.len, tr.len)
            assert np.array_equal(got_delta, delta)
            assert np.array_equal(delta, np.where(term != 0, 0, bn) - av)      # td_evaluate's expression
    return tr


def check_update(lib, tr, deltas, lr_shift, mode, net, tc=None):
    """host == reference for one trace update; returns (the reference's net, tc and trace)."""
    rnet, rtc, trace = net.copy(), None if tc is None else tc.copy(), {}
    if mode == 0:
        tref.trace_update(rnet, tr, deltas, lr_shift, trace)
        assert_tables_equal(host_trace_update(lib, tr, deltas, lr_shift, 0, net)[:1], (rnet.weights,))
    else:
        tref.tc_trace_update(rnet, rtc, tr, deltas, lr_shift, mode, trace)
        assert_tables_equal(host_trace_update(lib, tr, deltas, lr_shift, mode, net, tc), (rnet.weights, rtc.err, rtc.mag_i64()))
    return rnet, rtc, trace


def test_push_len_every_byte(ht):
    """All 256 old bytes, every H, both flags: push is total.  0x7f and 0xff are the garbage bytes the definition names."""
    trace = {}
    for H in range(1, 9):
        for old in range(256):
            for term in (0, 1, 0xff):
                want = tref.push_len(old, H, term, trace)
                assert ht.ntuple_check_push_len(old, H, term) == want, (old, H, term)
                assert 1 <= (want & 0x7f) <= H and bool(want & 0x80) == bool(term)
            assert ht.ntuple_check_len(old, H) == min(old & 0x7f, H)
    assert trace["garbage"] > 0 and trace["ended"] > 0 and trace["saturate"] > 0
    assert tref.push_len(0x7f, 4, 0) == 4 and tref.push_len(0xff, 4, 0) == 1 and tref.push_len(0xff, 4, 1) == 0x81
    assert tref.push_len(0x83, 8, 0) == 1 and tref.push_len(3, 8, 0) == 4 and tref.push_len(8, 8, 1) == 0x88


@pytest.mark.parametrize("H", [1, 2, 3, 4, 8])
def test_twelve_pushes_wrap_fill_and_clear(ht, H):
    n, trace = 23, {}
    tr = filled(n, H, 32768, 12, 11 + H, trace, ht)
    assert trace["pushes"] == 12 > H and trace["wrap"] >= 1                 # the ring wraps
    assert trace["term"] > n and trace["ended"] > n                         # the flag is set and consumed by the next push
    if H <= 4:
        assert trace["saturate"] > 0 and (tr.len & 0x7f).max() == H          # len saturates at H
    assert (tr.len & 0x7f).min() == 1 and len(set((tr.len & 0x7f).tolist())) > (1 if H > 1 else 0)
    assert tr.slot == 11 % H


def test_never_ending_boards_saturate_at_8(ht):
    trace = {}
    tr = filled(23, 8, 65536, 12, 5, trace, ht)
    assert trace["saturate"] > 0 and (tr.len[6::7] == 8).all()


def test_garbage_len_bytes(ht):
    """0x7f and 0xff in len: the update reads min(low bits, H) slots, the next push restarts (0xff) or saturates (0x7f)."""
    n, H = 12, 4
    tr = filled(n, H, 32768, 6, 21)
    tr.len[::2], tr.len[1::2] = 0x7f, 0xff
    net = random_net(TUPLES_17x4, 22, lo=-1000, hi=1000)
    deltas = np.random.default_rng(23).integers(1 << 20, 1 << 24, n)
    _, _, trace = check_update(ht, tr, deltas, 2, 0, net)
    assert trace.get("short", 0) == 0 and trace["items"] == H * n
    check_update(ht, tr, deltas, 2, 3, net, preload(net, 24))
    ptrace = {}
    after, av, bn, term = push_inputs(n, 1, 25)[0]
    got, _ = host_push(ht, tr, after, av, bn, term)
    tref.push(tr, after, av, bn, term, ptrace)
    assert ptrace["garbage"] == n and ptrace["ended"] == n // 2 and np.array_equal(got.len, tr.len)
    assert set((tr.len[::2] & 0x7f).tolist()) == {4} and set((tr.len[1::2] & 0x7f).tolist()) == {1}


def test_decay_for_every_k(ht):
    for lam in LAMS + (2, 255, 256, 257, 40000, 65534):
        for k in range(8):
            assert ht.ntuple_check_decay(lam, k) == tref.decay(lam, k), (lam, k)
    assert [tref.decay(65536, k) for k in range(8)] == [65536] * 8
    assert [tref.decay(0, k) for k in range(4)] == [65536, 0, 0, 0]
    assert [tref.decay(1, k) for k in range(4)] == [65536, 1, 0, 0]
    assert [tref.decay(32768, k) for k in range(8)] == [65536 >> k for k in range(8)]
    assert [tref.decay(65535, k) for k in range(4)] == [65536, 65535, 65534, 65533]     # floors: one less each time


def test_dk_edges(ht):
    deltas = [3, -3, 1, -1, 2, -2, 0, 12345, -12345, 1 << 40, -(1 << 40), (1 << 40) + 1, -(1 << 40) - 1, INT64_MAX, INT64_MIN,
              (1 << 31) - 1, -(1 << 31), 65535, -65537]
    for d in deltas:
        for lam in LAMS:
            for k in range(8):
                assert ht.ntuple_check_dk(d, lam, k) == tref.d_k(d, lam, k), (d, lam, k)
    # d_k reaches 0 for k > 0 while d_0 != 0
    assert [tref.d_k(3, 32768, k) for k in range(3)] == [3, 1, 0] and tref.d_k(5, 0, 1) == 0 and tref.d_k(5, 1, 1) == 0
    # the negative floor: d = -1 stays -1 as long as p_k > 0, and -3 decays to -1, not to 0
    assert [tref.d_k(-1, 32768, k) for k in range(8)] == [-1] * 8 and [tref.d_k(-3, 32768, k) for k in range(4)] == [-3, -2, -1, -1]
    assert tref.d_k(-1, 1, 1) == -1 and tref.d_k(-1, 1, 2) == 0 == tref.d_k(-1, 0, 1)      # p_k == 0 gives 0
    # the clamp, and lam = 1.0 keeps it
    assert tref.d_k(INT64_MAX, 65536, 7) == 1 << 40 == tref.d_k((1 << 40) + 1, 65536, 0) and tref.d_k(INT64_MIN, 65536, 7) == -(1 << 40)
    assert tref.d_k(INT64_MAX, 32768, 3) == 1 << 37 and tref.d_k(INT64_MIN, 65535, 1) == -(1 << 40) + (1 << 24)


def test_split_is_k_major(ht):
    for n, H in ((1, 1), (1, 8), (63, 2), (65, 8), (257, 3), ((1 << 32) - 256, 8), ((1 << 25) + 3, 8)):
        for item in {0, 1, n - 1, n, n + 1, 2 * n - 1, H * n - 1, (H - 1) * n, (H // 2) * n + n // 2}:
            if item < H * n:
                assert ht.ntuple_check_split(item, n, H) == (item // n) << 32 | item % n, (item, n, H)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("H, lam", [(1, 32768), (2, 65536), (4, 32768), (8, 65535), (8, 1), (4, 0)])
def test_whole_updates(ht, mode, H, lam):
    n = 40
    ptrace = {}
    tr = filled(n, H, lam, 12, 31 + H, ptrace)
    net = random_net(TUPLES_17x4, 32, lo=-(1 << 30), hi=1 << 30)
    tc = preload(net, 33, tr.hist[tr.slot, :8]) if mode else None
    deltas = trace_deltas(n, 34)
    rnet, rtc, trace = check_update(ht, tr, deltas, 0, mode, net, tc)
    assert trace["zero"] >= 4 and trace["clamp_d"] >= 4 and trace["items"] > 0
    if H > 1:
        assert trace["short"] > 0                                            # some boards have short histories
        assert (trace["items"] > n - trace["zero"]) == (lam > 0)             # lam = 0: only k = 0 has anything to do
    if H >= 4 and lam in (32768, 1):
        assert trace["dk_zero"] > 0                                          # d_k reaches 0 for k > 0 while d_0 != 0
    if H > 1 and lam >= 32768:
        assert trace["neg_floor"] > 0                                        # -1 stays -1
    if mode in (0, 1, 3):
        assert trace["sat"] > 0 and (rnet.weights != net.weights).any()      # int32 saturation at lr_shift 0
    if mode == 2:
        assert (rnet.weights == net.weights).all() and (rtc.err != tc.err).any()
    if mode == 1:
        assert (rtc.err == tc.err).all() and (rtc.mag == tc.mag).all()


def test_saturation_at_lr_shift_0_from_every_slot(ht):
    """|delta| > 2^31 - 1 with lam = 1: d_k = d for every k, and every step clips to the int32 range."""
    n, H = 6, 4
    tr = filled(n, H, 65536, 4, 41)
    tr.len[:] = H
    net = ref.Net(TUPLES_17x4, 10)
    deltas = [1 << 40, -(1 << 40), INT64_MAX, INT64_MIN, 1 << 31, -(1 << 31) - 1]
    rnet, _, trace = check_update(ht, tr, deltas, 0, 0, net)
    assert trace["sat"] == trace["items"] == H * n                          # 2^31 is the first step to clip, -2^31 - 1 too
    assert (rnet.weights != 0).any()


def test_zero_deltas_leave_all_three_tables_untouched(ht):
    n = 30
    tr = filled(n, 4, 32768, 7, 51)
    net = random_net(TUPLES_17x4, 52)
    tc = preload(net, 53)
    for mode in (0, 1, 2, 3):
        rnet, rtc, trace = check_update(ht, tr, [0] * n, 0, mode, net, tc if mode else None)
        assert trace["zero"] == n and trace.get("items", 0) == 0 and (rnet.weights == net.weights).all()
        if mode:
            assert (rtc.err == tc.err).all() and (rtc.mag == tc.mag).all()


@pytest.mark.parametrize("H, lam", [(1, 0), (1, 32768), (1, 65536), (4, 0), (8, 0)])
def test_h_1_and_lam_0_are_the_one_step_updates(ht, H, lam):
    n = 40
    tr = filled(n, H, lam, 12, 61)
    last = tr.hist[tr.slot]
    net = random_net(TUPLES_17x4, 62, lo=-(1 << 20), hi=1 << 20)
    tc = preload(net, 63, last[:8])
    small = np.clip(trace_deltas(n, 64), -(1 << 40), 1 << 40)              # the TD equality needs |delta| <= 2^40
    assert (np.abs(small) == 1 << 40).any() and (small < 0).any() and (small == 0).any()
    for lr_shift in (0, 7):
        one = net.copy()
        ref.update(one, last, small, lr_shift)
        assert_tables_equal(host_trace_update(ht, tr, small, lr_shift, 0, net)[:1], (one.weights,))
        check_update(ht, tr, small, lr_shift, 0, net)
        wide = trace_deltas(n, 65)                                          # the TC equality holds for every delta
        assert (np.abs(wide.astype(object)) > 1 << 40).any()
        for phases in (1, 2, 3):
            one, one_tc = net.copy(), tc.copy()
            tcref.tc_update(one, one_tc, last, wide, lr_shift, phases)
            assert_tables_equal(host_trace_update(ht, tr, wide, lr_shift, phases, net, tc), (one.weights, one_tc.err, one_tc.mag_i64()))
    # beyond the clamp the TD forms differ, as the definition says: the one-step update does not clamp
    big = np.zeros(n, np.int64)
    big[0] = 1 << 45
    one, two = net.copy(), net.copy()
    ref.update(one, last, big, 20)
    tref.trace_update(two, tr, big, 20)
    assert (one.weights != two.weights).any()


def test_same_entry_from_two_slots_counts_twice(ht):
    """One board pushed into every slot: each of its entries is reached H times, eight-fold for the all-empty board."""
    n, H = 2, 4
    tr = tref.Trace(n, H, 65536)
    boards = np.array([[0] * 16, [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 0]], np.uint8)
    for _ in range(H):
        tref.push(tr, boards, [0, 0], [0, 0], [0, 0])
    net = ref.Net(TUPLES_17x4, 10)
    rnet, rtc, trace = check_update(ht, tr, [1000, -64], 3, 3, net, tcref.TC(net))
    assert trace["multi"] > 0 and rnet.weights[0, 0] == H * 8 * (1000 >> 3) and rtc.err[0, 0] == H * 8000 == rtc.mag[0, 0]
    rnet, _, _ = check_update(ht, tr, [1000, -64], 3, 0, net)
    assert rnet.weights[0, 0] == H * 8 * (1000 >> 3)


def _one_slot_history(boards):
    """A trace of depth 1 that holds ``boards``: the items of its update are the boards themselves."""
    tr = tref.Trace(len(boards), 1, 32768)
    tref.push(tr, boards, np.zeros(len(boards), np.int64), np.zeros(len(boards), np.int64), np.zeros(len(boards), np.uint8))
    assert tr.slot == 0 and (tr.len == 1).all() and np.array_equal(tr.hist[0], boards)
    return tr


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_board_items_and_one_slot_trace_items_give_the_same_tables(ht, mode):
    """The update entry point over the board source and over the trace source with H = 1: the same per-item operations
    on the same boards, so all three tables agree as long as no delta passes the clamp."""
    n = 64
    boards = mixed_boards(n, 81)
    rng = np.random.default_rng(82)
    deltas = rng.integers(-(1 << 20), 1 << 20, n) << rng.integers(0, 21, n)
    deltas[::11] = 0
    deltas[1:5] = [1 << 40, -(1 << 40), 1, -1]
    assert np.abs(deltas).max() == 1 << 40 and (deltas < 0).any() and (deltas > 0).any() and (deltas == 0).sum() >= 6
    net = random_net(TUPLES_17x4, 83, lo=-(1 << 30), hi=1 << 30)
    tc = preload(net, 84, boards[:8]) if mode else None
    tr = _one_slot_history(boards)
    for lr_shift in (0, 6):
        got_boards = host_update(ht, boards, deltas, lr_shift, mode, net, tc)
        got_trace = host_trace_update(ht, tr, deltas, lr_shift, mode, net, tc)
        assert_tables_equal(got_boards, got_trace)
        assert (got_boards[0] != net.weights).any() == (mode != 2)


def test_only_the_plain_td_form_is_unclamped(ht):
    """Past 2^40 the two sources differ in mode 0, as the definition says: the board source shifts delta as it is, the
    trace source d_0 = clamp(delta).  Each equals its Python reference."""
    n = 64
    boards = mixed_boards(n, 85)
    deltas = np.random.default_rng(86).integers(-(1 << 30), 1 << 30, n)
    deltas[[3, 9, 20, 41]] = [(1 << 40) + 1, -(1 << 45), tcref.INT64_MAX, tcref.INT64_MIN]
    assert (np.abs(deltas.astype(object)) > 1 << 40).sum() == 4
    net = random_net(TUPLES_17x4, 87, lo=-1000, hi=1000)
    tr = _one_slot_history(boards)
    lr_shift = 12                                                        # 2^45 >> 12 does not saturate: the clamp shows
    got_boards = host_update(ht, boards, deltas, lr_shift, 0, net)[0]
    got_trace = host_trace_update(ht, tr, deltas, lr_shift, 0, net)[0]
    one, two = net.copy(), net.copy()
    ref.update(one, boards, deltas, lr_shift)
    tref.trace_update(two, tr, deltas, lr_shift)
    assert (got_boards != got_trace).any()
    assert_tables_equal((got_boards, got_trace), (one.weights, two.weights), names=("board source", "trace source"))


def test_out_of_range_arguments_are_refused(ht):
    z = np.zeros(64, np.int64)
    p = z.ctypes.data
    ok = dict(shift=3, mode=0, T=4, L=4, H=4, lam=100, slot=0)
    for bad in (dict(T=0), dict(T=9), dict(L=0), dict(L=7), dict(shift=41), dict(mode=4), dict(H=0), dict(H=9), dict(lam=65537),
                dict(slot=4)):
        a = dict(ok, **bad)
        assert ht.ntuple_check_trace_update(1, p, a["shift"], a["mode"], raw_desc(a["T"], a["L"]), p, p, p, a["H"], a["lam"], p, p, a["slot"]) == -1
    assert ht.ntuple_check_push(p, p, p, p, 1, 0, p, p, 0, p) == -1 and ht.ntuple_check_push(p, p, p, p, 1, 9, p, p, 0, p) == -1
    assert ht.ntuple_check_push(p, p, p, p, 1, 4, p, p, 4, p) == -1


@pytest.mark.parametrize("H, lam", [(1, 32768), (4, 32768), (8, 65536)])
def test_the_array_form_of_the_reference_is_the_scalar_one(H, lam):
    """ntuple_trace_ref.trace_update_np (used to replay long runs) against trace_update, saturation and wrap included."""
    n = 40
    tr = filled(n, H, lam, 12, 71)
    for lr_shift, lo in ((0, -(1 << 31)), (6, -1000)):
        net = random_net(TUPLES_17x4, 72, lo=lo, hi=-lo)
        a, b, trace = net.copy(), net.copy(), {}
        tref.trace_update(a, tr, trace_deltas(n, 73), lr_shift, trace)
        tref.trace_update_np(b, tr, trace_deltas(n, 73), lr_shift)
        assert trace["items"] > (n if H > 1 else n // 2) and (lr_shift or trace["sat"] > 0 and trace["wrap32"] > 0)
        assert_tables_equal((b.weights,), (a.weights,))
