"""CPU: the temporal-coherence code of g2048_device.h -- the header the kernels are compiled from -- built for the host
(tests/host_ntuple/ntuple_check.cpp, g++) and compared bit for bit with the pure-Python reference
tests/ntuple_tc_ref.py.  Every test shows from the reference's own trace (never from the code under test) that its input
reaches the edge it names."""
import random

import numpy as np
import pytest

import ntuple_ref as ref
import ntuple_tc_ref as tcref
from analysis_helpers import random_boards, trajectory_boards
from ntuple_helpers import TUPLES_17x4, host_update, load_host_ntuple, random_net, raw_desc
from ntuple_tc_helpers import EDGE_PAIRS, assert_tables_equal, preload

INT32_MAX, INT32_MIN = (1 << 31) - 1, -(1 << 31)
INT64_MAX, INT64_MIN = (1 << 63) - 1, -(1 << 63)
U64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def ht():
    return load_host_ntuple()


def check_update(lib, boards, deltas, lr_shift, phases, net, tc):
    """host == reference for one update; returns (the reference's net, tc and trace)."""
    rnet, rtc, trace = net.copy(), tc.copy(), {}
    tcref.tc_update(rnet, rtc, boards, deltas, lr_shift, phases, trace)
    assert_tables_equal(host_update(lib, boards, deltas, lr_shift, phases, net, tc), (rnet.weights, rtc.err, rtc.mag_i64()))
    return rnet, rtc, trace


def test_rate_edges(ht):
    table = {
        "never updated": [(0, 0), (123, 0), (INT64_MIN, 0)],
        "E = 0": [(0, 1), (0, 1 << 40), (0, U64)],
        "|E| = A": [(1, 1), (-1, 1), (77, 77), (-(1 << 40), 1 << 40), (INT64_MAX, INT64_MAX), (INT64_MIN, 1 << 63)],
        "|E| = A - 1": [(0, 1), (76, 77), (-65535, 65536), (65536, 65537), ((1 << 32) - 2, (1 << 32) - 1), (-(1 << 32) + 1, 1 << 32),
                        (1 << 32, (1 << 32) + 1), (INT64_MAX, 1 << 63), (-INT64_MAX + 1, INT64_MAX)],
        "A around 2^32, 2^63, 2^64": [(e, a) for a in ((1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 63, U64)
                                      for e in (1, -1, 65535, 1 << 16, -(1 << 31), (1 << 32) - 1, a >> 1, -(a >> 2), min(a, INT64_MAX),
                                                INT64_MIN)],
        "|E| > A": [(2, 1), (-(1 << 40), 3), (INT64_MAX, 1 << 32), (INT64_MIN, 1), (INT64_MIN, INT64_MAX)],
    }
    assert tcref.rate(0, 0) == tcref.rate(INT64_MIN, 0) == 65536 and tcref.rate(0, 5) == 0 and tcref.rate(-9, 9) == 65536
    assert tcref.rate(76, 77) == (76 << 16) // 77 and tcref.rate(2, 1) == 65536 and tcref.rate(INT64_MIN, U64) == 32768
    for name, pairs in table.items():
        trace = {}
        for e, a in pairs:
            assert ht.ntuple_check_tc_rate(e, a) == tcref.rate(e, a, trace), (name, e, a)
        if name == "never updated":
            assert trace["rate1"] == len(pairs) and "k" not in trace
        elif name == "E = 0":
            assert trace["rate0"] == len(pairs) and trace["k"] == 2
        elif name == "|E| = A":
            assert trace["rate1"] == len(pairs) and trace["k"] == 3
        elif name == "|E| = A - 1":
            assert trace["rate1"] <= 4 and trace["k"] >= 4     # (A - 1) >> k can equal A >> k: rate 1.0 is right there
        elif name == "|E| > A":
            assert trace["clamp_m"] == len(pairs) == trace["rate1"]
        else:
            assert trace["k"] == 40 and trace["clamp_m"] == 3 and 0 < trace["rate1"] < len(pairs) and trace["rate0"] > 0


def test_rate_random_pairs(ht):
    """About 10 000 pairs with bitlen(A) uniform in 1..64, |E| uniform below, at and (rarely) above A."""
    rng = random.Random(1)
    trace, n = {}, 10000
    for _ in range(n):
        bits = rng.randint(1, 64)
        a = rng.getrandbits(bits) | 1 << (bits - 1)
        kind = rng.randrange(8)
        e = a if kind == 0 else (a + rng.randint(1, 1000) if kind == 1 else rng.randint(0, a))
        e = min(e, 1 << 63)
        e = -e if (e == 1 << 63 or rng.randrange(2)) else e
        assert a.bit_length() == bits
        assert ht.ntuple_check_tc_rate(e, a) == tcref.rate(e, a, trace), (e, a)
    assert trace["k"] > n // 3 and trace["clamp_m"] > 100 and trace["rate1"] > 1000 and trace["rate0"] > 0


def test_rate_small_divisors_exhaustive(ht):
    """Every (m, A) with A <= 300, and every m for a few A near powers of two: the quotient's correction step."""
    for a in range(1, 301):
        for m in range(0, a + 1):
            assert ht.ntuple_check_tc_rate(m, a) == (m << 16) // a, (m, a)
    for a in (65535, 65536, 65537, (1 << 24) - 1, (1 << 24) + 1, (1 << 32) - 1, (1 << 32) - 65535):
        for m in list(range(0, 2000)) + list(range(a - 2000, a + 1)) + list(range(a // 2 - 1000, a // 2 + 1000)):
            assert ht.ntuple_check_tc_rate(-m, a) == (m << 16) // a, (m, a)


def test_step_edges(ht):
    cases = [(d, r, s) for d in ((1 << 40), -(1 << 40), (1 << 40) + 1, -(1 << 40) - 1, INT64_MIN, INT64_MAX, 12345, -12345, 1, -1, 0)
             for r in (0, 1, 32768, 65535, 65536) for s in (0, 5, 40)]
    trace = {}
    for d, r, s in cases:
        assert ht.ntuple_check_tc_step(d, r, s) == tcref.step(d, r, s, trace), (d, r, s)
    assert trace["sat"] > 0
    # the clamp: 2^40 + 1 and INT64_MAX step as 2^40 does
    assert tcref.step((1 << 40) + 1, 65536, 10) == tcref.step(INT64_MAX, 65536, 10) == tcref.step(1 << 40, 65536, 10) == 1 << 30
    assert tcref.step(-(1 << 40) - 1, 65536, 10) == tcref.step(INT64_MIN, 65536, 10) == -(1 << 30)
    # saturation: lr_shift 0, rate 1.0, |d| >= 2^31 -- 2^31 is the first step to clip, -2^31 the last to fit
    assert tcref.step(1 << 31, 65536, 0) == INT32_MAX and tcref.step(-(1 << 31), 65536, 0) == INT32_MIN == -(1 << 31)
    assert tcref.step((1 << 31) - 1, 65536, 0) == INT32_MAX and tcref.step(-(1 << 31) - 1, 65536, 0) == INT32_MIN
    for d in (1 << 31, -(1 << 31), (1 << 31) - 1, -(1 << 31) - 1, 1 << 40, -(1 << 40)):
        assert ht.ntuple_check_tc_step(d, 65536, 0) == tcref.step(d, 65536, 0)
    # negative products floor: -1 * 1 >> 16 is -1, not 0; the positive twin is 0
    assert tcref.step(-1, 1, 0) == -1 and tcref.step(1, 1, 0) == 0 and tcref.step(-1, 65536, 40) == -1
    assert ht.ntuple_check_tc_step(-1, 1, 0) == -1 and ht.ntuple_check_tc_step(1, 1, 0) == 0 and ht.ntuple_check_tc_step(-1, 65536, 40) == -1
    # lr_shift 40: the largest product, 2^56, becomes 1
    assert tcref.step(1 << 40, 65536, 40) == 1 == ht.ntuple_check_tc_step(1 << 40, 65536, 40)
    assert all(tcref.step(0, r, s) == 0 == ht.ntuple_check_tc_step(0, r, s) for r in (0, 65536) for s in (0, 40))


BOARDS = np.concatenate([random_boards(40, 2), trajectory_boards(every=211)[:40]])


def edge_deltas(n, seed):
    """Mixed-sign deltas of every size up to beyond the clamp, with zeros."""
    rng = np.random.default_rng(seed)
    d = rng.integers(-(1 << 20), 1 << 20, n) << rng.integers(0, 24, n)
    d[::9] = 0
    d[1::13] = [(1 << 40) + 1, -(1 << 40) - 1, INT64_MAX, INT64_MIN, 1 << 40, -(1 << 40), 1, -1][:len(d[1::13])]
    return d


@pytest.mark.parametrize("phases", [1, 2, 3])
@pytest.mark.parametrize("lr_shift", [0, 5])
def test_whole_updates_with_preloaded_accumulators(ht, phases, lr_shift):
    net = random_net(TUPLES_17x4, 3, lo=-(1 << 30), hi=1 << 30)
    tc = preload(net, 4, BOARDS[:8])
    deltas = edge_deltas(len(BOARDS), 5)
    rnet, rtc, trace = check_update(ht, BOARDS, deltas, lr_shift, phases, net, tc)
    assert trace["zero"] >= 8 and trace["clamp_d"] >= 4 and trace["multi"] > 0
    if phases & 1:
        assert trace["k"] > 100 and trace["rate0"] > 0 and trace["rate1"] > 100 and trace["clamp_m"] > 0 and trace["zero_step"] > 0
        assert trace["sat"] > 0 and (rnet.weights != net.weights).any()
    else:
        assert (rnet.weights == net.weights).all()
    if phases & 2:
        assert (rtc.err != tc.err).any() and (rtc.mag != tc.mag).any()
    else:
        assert (rtc.err == tc.err).all() and (rtc.mag == tc.mag).all()


def test_phase_w_then_phase_a_is_phases_3(ht):
    net = random_net(TUPLES_17x4, 6, lo=-1000, hi=1000)
    tc = preload(net, 7, BOARDS[:4])
    deltas = edge_deltas(len(BOARDS), 8)
    w3, e3, m3 = host_update(ht, BOARDS, deltas, 5, 3, net, tc)
    w1, e1, m1 = host_update(ht, BOARDS, deltas, 5, 1, net, tc)
    w2, e2, m2 = host_update(ht, BOARDS, deltas, 5, 2, net, tc)
    assert np.array_equal(w1, w3) and np.array_equal(e2, e3) and np.array_equal(m2, m3)
    assert np.array_equal(w2, net.weights) and np.array_equal(e1, tc.err) and np.array_equal(m1, tc.mag_i64())


def test_all_empty_and_symmetric_board_multiplicity_8(ht):
    """The all-empty board reads entry 0 of every table eight times; a board of one repeated exponent reads one entry of
    every table eight times.  The weight moves by 8 steps and the accumulators by 8 d."""
    net = ref.Net(TUPLES_17x4, 10)
    boards = np.array([[0] * 16, [3] * 16], np.uint8)
    for b in boards:
        hits = tcref.hits_of(b, net)
        assert len(hits) == 40 and len(set(hits)) == 5 and all(hits.count(h) == 8 for h in set(hits))
    tc = tcref.TC(net)
    rnet, rtc, trace = check_update(ht, boards, [1000, -64], 3, 3, net, tc)
    assert trace["multi"] == 10 and trace["rate1"] == 80
    assert rnet.weights[0, 0] == 8 * (1000 >> 3) and rtc.err[0, 0] == 8000 == rtc.mag[0, 0]
    assert rnet.weights[2, 0x3333] == 8 * (-64 >> 3) and rtc.err[2, 0x3333] == -512 and rtc.mag[2, 0x3333] == 512
    # a second call sees the first one's accumulators: err and mag agree, the rate stays 1.0; an opposite delta halves it
    net2, tc2, trace = check_update(ht, boards[:1], [-8000], 0, 3, rnet, rtc)
    assert trace["rate1"] == 40 and tc2.err[0, 0] == 8000 - 64000 and tc2.mag[0, 0] == 8000 + 64000
    _, _, trace = check_update(ht, boards[:1], [1 << 16], 0, 1, net2, tc2)
    assert trace.get("rate1", 0) == 0 and tcref.rate(-56000, 72000) == (56000 << 16) // 72000


def test_zero_deltas_leave_all_three_tables_untouched(ht):
    net = random_net(TUPLES_17x4, 9)
    tc = preload(net, 10)
    for phases in (1, 2, 3):
        rnet, rtc, trace = check_update(ht, BOARDS, [0] * len(BOARDS), 0, phases, net, tc)
        assert trace["zero"] == len(BOARDS)
        assert (rnet.weights == net.weights).all() and (rtc.err == tc.err).all() and (rtc.mag == tc.mag).all()


def test_accumulators_wrap_mod_2_64(ht):
    net = ref.Net(TUPLES_17x4, 10)
    tc = tcref.TC(net)
    board = np.array([[0] * 16], np.uint8)
    tc.err[:, 0], tc.mag[:, 0] = INT64_MAX - 3, U64 - 3
    _, rtc, _ = check_update(ht, board, [1], 0, 2, net, tc)
    assert rtc.err[0, 0] == INT64_MIN + 4 and rtc.mag[0, 0] == 4


def test_out_of_range_arguments_are_refused(ht):
    z = np.zeros(64, np.int64)
    p = z.ctypes.data
    for T, L, shift, phases in ((0, 4, 3, 3), (9, 4, 3, 3), (4, 0, 3, 3), (4, 7, 3, 3), (4, 4, 41, 3), (4, 4, 3, 0), (4, 4, 3, 4)):
        assert ht.ntuple_check_tc_update(p, 1, p, shift, phases, raw_desc(T, L), p, p, p) == -1


def test_edge_pairs_cover_the_rate(ht):
    trace = {}
    for e, a in EDGE_PAIRS:
        assert ht.ntuple_check_tc_rate(e, a) == tcref.rate(e, a, trace)
    assert trace["k"] >= 6 and trace["rate0"] >= 3 and trace["rate1"] >= 6 and trace["clamp_m"] >= 3
