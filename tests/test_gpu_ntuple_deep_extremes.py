"""GPU: the deep and the adaptive n-tuple search kernels where the header's range argument matters:
weights at INT32_MIN / INT32_MAX, F = 0 and 16 and tiles of 2^27 .. 2^29, so that |V| reaches 2^37, a move gains up to 2^30 +
2^29, values reach 2^48 and root chance sums 2^53 -- against the pure-Python reference tests/ntuple_search_ref.py, bit for bit.

Where an expected value comes from.  The reference (ntuple_deep_helpers.reference_rows) wherever it takes a few seconds at
most: every board at depths 0..2, DEAD_ENDS and SYMMETRIC at every depth, MERGING and MIRRORED at depth 3 with one tuple, HUGE at
depth 3 under one network.  Everything else is composed (anchored_search): the top chance sum and its floor division in Python
integers over the values the GPU gives for the children one level down, and of those children the quarter with the fewest
empty cells (the cheapest references) and every child without a legal move is itself compared, in the same call, with the
reference (depth 2) or with the same construction one level further down (depth 3): GPU depth 4 <- GPU depth 3 <- GPU depth
2 <- reference.  No expected value comes from the call under test.

Every test shows from the reference (never from the code under test) that its input reaches the edge it names.  Not reached:
  * "a root chance sum below -2^52 under the min fill": gains are never negative and V >= -2^37, so no chance sum lies below
    -150 * 2^37 > -2^45 under any network; the near-full boards here reach -2^40.3 (asserted: below -2^40).
  * HUGE at depth 4 straight against the reference: measured 11 s at depth 3 with one tuple (51 s with eight), and depth 4 is
    about 30 times that; SYMMETRIC, DEAD_ENDS (0.6 s each at depth 4) and the anchored composition stand in.
  * one launch with one-empty boards at depths 3 AND 4: the depth is a function of the empty cells alone, so the mixed launch
    has its one-empty boards at depth 4 and its two-empty boards at depth 3.
  * depth 3 of the two-empty boards with eight tuples: the anchor alone (a quarter of 40 children at 1.7 s each) is 17 s a
    network; they run with one tuple, and HUGE with eight under the random fill (8 s).
  * values on both sides of -2^36 at depth 4: under the min fill the maximiser walks into the dead ends, and the lowest depth-4
    value of the boards the reference affords is -0.82 * 2^36 (depths 1..3 are asserted).
  * a negative inexact division at the fold level under the random fill with one tuple (none on the affordable boards; the
    min fill has them at every depth, asserted), and a fold sum above 2^53 on a residue where one unit changes the quotient:
    a build whose fold divides acc through a double passes this module.  The root's division has such a sum (SENSITIVE).

CPU time of the reference work on one core: 2 .. 5 s for a deep-search case, 8 .. 15 s for the three that carry HUGE with
eight tuples, HUGE straight from the reference, or the two-empty boards; 9 s for depth 4 of HUGE; about 75 s for the module,
30 s of wall time on the GPU host.  The device work is milliseconds.
"""
import numpy as np
import pytest

import ntuple_ref as ref
from analysis_helpers import g  # noqa: F401 (g: fixture)
from ntuple_adaptive_helpers import adaptive_np, constant
from ntuple_deep_helpers import (HUGE, ILLEGAL, LOW_STAGE, MERGING, SENSITIVE, SYMMETRIC, TURNED, TWO_EMPTY, anchored_search, cached, cleared, dev, dev_u32,
                                 device_net, engine_with, extreme_mixed_net, extreme_net, extreme_staged_net, fold_sums, implied_root_sums,
                                 kind_of, reference_rows, reference_trace, to_np)
from ntuple_search_helpers import assert_search_equal
from test_gpu_ntuple_shapes import DEAD_ENDS, MIRRORED, far_apart, ties

pytestmark = pytest.mark.gpu

UNIFORM = [(kind, F, T) for T in (8, 1) for kind in ("min", "max", "random") for F in (0, 16)]
BIG = np.concatenate([HUGE, TURNED, SYMMETRIC, TWO_EMPTY])      # the boards of 2^27 .. 2^29 tiles
CHEAP = np.concatenate([MERGING, DEAD_ENDS, MIRRORED, SYMMETRIC])


def net_of(case):
    return {"staged": extreme_staged_net, "mixed": extreme_mixed_net}[case]() if isinstance(case, str) else extreme_net(*case)


def same(a, b):
    return np.array_equal(np.asarray(a).reshape(-1), np.asarray(b).reshape(-1))


def direct_depth(case):
    """The deepest search of a board that comes straight from the reference under the network ``case`` (module docstring)."""
    one_tuple = not isinstance(case, str) and case[2] == 1

    def depth(b):
        if same(b, SYMMETRIC) or same(b, DEAD_ENDS[0]) or (same(b, DEAD_ENDS[1]) and one_tuple):
            return 4
        if same(b, DEAD_ENDS[1]) or (one_tuple and (same(b, MERGING) or same(b, MIRRORED))):
            return 3
        return 3 if case == ("max", 16, 1) and same(b, HUGE) else 2
    return depth


def gpu_lower(torch, net):
    """``lower`` of anchored_search on the device: evaluate, search(1), deep_search(2) and deep_search(3)."""
    def lower(kids, k):
        d = dev(torch, kids)
        r = net.evaluate(d) if k == 0 else net.search(d, 1) if k == 1 else net.deep_search(d, k)
        return r.action.cpu().numpy(), r.value.cpu().numpy()
    return lower


_expected, _stats = {}, {}


def expected(torch, g, case, boards, depth):
    """(action, value) of ``boards`` at ``depth`` under network ``case`` by anchored_search, every row made once per process:
    the constant schedules, the mixed launch and the deep search are checked against the same rows."""
    rnet = net_of(case)
    boards = np.asarray(boards, np.uint8).reshape(-1, 16)
    act, val = np.zeros(len(boards), np.uint8), np.zeros((len(boards), 4), np.int64)
    for i, b in enumerate(boards):
        key = case, depth, b.tobytes()
        if key not in _expected:
            a, v = anchored_search(b, depth, rnet, gpu_lower(torch, device_net(g, rnet)), direct_depth(case), _stats.setdefault((case, depth), {}))
            _expected[key] = a[0], v[0]
        act[i], val[i] = _expected[key]
    return act, val


def counts(stats):
    return {k: v for k, v in stats.items() if k != "totals"}


def first_of_the_largest(value):
    return np.where(value != ILLEGAL, value, ILLEGAL).argmax(1)


def check_ranges(boards, want, F):
    """Every root gain below 2^31, every legal value below 2^50 and every root chance sum below 2^58 in magnitude; the sums."""
    sums = implied_root_sums(boards, want[1], F)
    assert all(abs(s) < 1 << 58 for per in sums for s in per)
    return sums


def fold_level_negative_inexact(case, depth):
    """Some chance sum one level below the root of a depth-``depth`` search is negative and no multiple of its 10 E, by the
    reference: on DEAD_ENDS[0], or else on SYMMETRIC (computed once per network and depth)."""
    def make():
        return any(any(s < 0 and s % e != 0 for s, e in fold_sums(b, depth, net_of(case))) for b in (DEAD_ENDS[0], SYMMETRIC[0]))
    return cached(("fold level", case, depth), make)


# ------------------------------------------------------------------------------------------------ 1. deep search
def deep_boards(case, depth):
    """Near-full boards only.  HUGE runs under every network at depth 2 and under every one-tuple network at depth 3, where its
    anchor is 8 depth-2 references of 0.2 s; with eight tuples (1.3 s each) under the random fill at F = 16 alone.  TURNED and
    the two-empty boards (depth 3 only) run with one tuple under the random fill at F = 16."""
    if isinstance(case, str):
        return np.concatenate([CHEAP, LOW_STAGE, HUGE]) if depth == 2 else CHEAP
    kind, F, T = case
    full = case == ("random", 16, 1)
    if depth == 2:
        return np.concatenate([CHEAP, HUGE] + ([TURNED] if T == 1 else []))
    return np.concatenate([CHEAP] + ([HUGE] if T == 1 or (kind, F) == ("random", 16) else []) + ([TURNED, TWO_EMPTY, SENSITIVE] if full else []))


def both_deep_forms(g, torch, net, boards, depth, want, where, mask=None):
    assert_search_equal(to_np(net.deep_search(dev(torch, boards), depth)), want, boards, f"{where}, plain")
    eng = engine_with(g, boards)
    try:
        assert bool((eng.records()[:, 8:] > 31).any()), "inputs: the score-deficit bits are populated"
        assert_search_equal(to_np(eng.ntuple_deep_search(net, depth)), want, boards, f"{where}, engine")
        if mask is not None:
            got = to_np(eng.ntuple_deep_search(net, depth, active=dev_u32(torch, mask)))
            on = mask != 0
            assert_search_equal((got[0][on], got[1][on]), (want[0][on], want[1][on]), boards[on], f"{where}, masked")
            assert (got[0][~on] == 0).all() and (got[1][~on] == ILLEGAL).all()
    finally:
        eng.close()


@pytest.mark.parametrize("case", UNIFORM + ["staged", "mixed"], ids=str)
def test_deep_search_at_the_value_extremes(g, torch_cuda, case):
    torch = torch_cuda
    rnet = net_of(case)
    net = device_net(g, rnet)
    F = rnet.frac_bits
    for depth in (2, 3):
        boards = deep_boards(case, depth)
        want = expected(torch, g, case, boards, depth)
        sums = check_ranges(boards, want, F)
        trace, stats = reference_trace(rnet, depth), _stats[case, depth]
        print(f"{case} depth {depth}: {counts(stats)}, sums 2^{np.log2(max(abs(s) for per in sums for s in per)):.1f}, {trace if kind_of(rnet) == 0 else ''}")
        rows = ties(want[1])
        assert rows.any() and (want[0][rows] == first_of_the_largest(want[1][rows])).all(), "inputs: a root tie, the smallest direction"
        if isinstance(case, str):
            if depth == 2:      # (at depth 3 every leaf of LOW_STAGE holds an 8, and the second of them takes the reference 3.6 s)
                assert sum(c > 0 for c in trace["stage"].values()) >= 2, "inputs: leaves in two stages"
                assert max(abs(s) for per in sums for s in per) > 1 << 52
        else:
            kind, _, T = case
            assert trace.root_ties > 0 and trace.terminal_children > 0
            if kind in ("min", "random"):
                assert trace.negative_inexact > 0
            if kind == "min":
                assert fold_level_negative_inexact(case, depth), "inputs: a negative inexact division at the fold level"
            if kind == "min" and (F, T) == (0, 8):
                assert far_apart(want[1]).any() and min(s for per in sums for s in per) < -(1 << 40)
            if kind == "max" and F == 16:
                assert (want[1] > 1 << 47).any()
            if depth == 3 and case != ("max", 16, 1):
                assert stats["composed"] >= 1 and stats["anchored"] >= 3, "a composed board and its anchors"
            if case == ("random", 16, 1) and depth == 3:
                exact = stats["totals"][3, SENSITIVE.tobytes()]     # (by the composition: the GPU's depth-2 values, a quarter anchored)
                assert any(t > 1 << 53 and int(float(t)) // e != t // e for _, _, t, e in exact), "inputs: a root sum that a double divides wrongly"
            if case == ("max", 16, 1) and depth == 3:      # HUGE straight from the reference, as tests/test_ntuple_deep_host.py has it
                huge = sums[len(CHEAP)]
                assert same(boards[len(CHEAP)], HUGE) and len(huge) == 4 and min(huge) > 1 << 52 and max(huge) > 1 << 53
        both_deep_forms(g, torch, net, boards, depth, want, f"{case}, depth {depth}",
                        mask=(np.arange(len(boards)) % 3 != 1).astype(np.uint32) * 7 if case == ("random", 16, 1) else None)


# ------------------------------------------------------------------------------------------------ 2. adaptive search
ADAPTIVE = [("random", 16, 1), ("min", 16, 1), ("min", 0, 8)]
ONE_EMPTY = np.concatenate([HUGE, TURNED, SYMMETRIC, MERGING])


def adaptive_boards(case, depth):
    """The one-empty boards, and DEAD_ENDS (full) for the dead children and the far-apart values.  At depth 4 HUGE runs under the
    random fill alone (its anchor chain is 8 x 8 depth-2 references), MERGING (small values, 19 s) and TURNED not at all; with
    eight tuples HUGE and TURNED stop at depth 2 and depth 4 has DEAD_ENDS[0] and SYMMETRIC, straight from the reference."""
    kind, F, T = case
    if T == 8:
        return np.concatenate([DEAD_ENDS[:1], SYMMETRIC] + ([DEAD_ENDS[1:], MERGING] if depth <= 3 else []) + ([HUGE, TURNED] if depth <= 2 else []))
    if depth == 4:
        return np.concatenate([DEAD_ENDS, SYMMETRIC] + ([HUGE] if kind == "random" else []))
    return np.concatenate([DEAD_ENDS, ONE_EMPTY] + ([SENSITIVE] if depth == 3 and kind == "random" else []))


def both_adaptive_forms(g, torch, net, boards, schedule, want, depths, where):
    for form in ("plain", "engine"):
        eng = engine_with(g, boards) if form == "engine" else None
        try:
            got = adaptive_np(net.adaptive_search(dev(torch, boards), schedule) if eng is None else eng.ntuple_adaptive_search(net, schedule))
        finally:
            if eng is not None:
                eng.close()
        assert_search_equal(got[:2], want, boards, f"{where}, {form}")
        assert got[2].tolist() == list(depths)


@pytest.mark.parametrize("depth", range(5))
@pytest.mark.parametrize("case", ADAPTIVE, ids=str)
def test_adaptive_search_constant_schedules_at_the_value_extremes(g, torch_cuda, case, depth):
    torch = torch_cuda
    rnet = net_of(case)
    net = device_net(g, rnet)
    kind, F, T = case
    boards = adaptive_boards(case, depth)
    want = expected(torch, g, case, boards, depth)
    sums = check_ranges(boards, want, F) if depth else None
    stats = _stats[case, depth]
    print(f"{case} depth {depth}: {counts(stats)}" + (f", sums 2^{np.log2(max(abs(s) for per in sums for s in per)):.1f}, {reference_trace(rnet, depth)}" if depth else ""))
    legal = want[1] != ILLEGAL
    assert legal.any(1).all() and (np.abs(want[1][legal]) < 1 << 50).all()
    rows = ties(want[1])
    assert rows.any() and (want[0][rows] == first_of_the_largest(want[1][rows])).all(), "inputs: a root tie, the smallest direction"
    if depth >= 1:
        trace = reference_trace(rnet, depth)
        assert trace.terminal_children > 0 and trace.root_ties > 0 and trace.negative_inexact > 0
    if kind == "min" and (depth == 3 or (depth == 4 and T == 1)):
        assert fold_level_negative_inexact(case, depth), "inputs: a negative inexact division at the fold level"
    if (kind, F, T) == ("min", 0, 8):
        leaf = ref.value(ref.move(ref.plain(SYMMETRIC[0]), 0)[0], rnet)
        assert leaf == -(1 << 37), "inputs: V at its bound"
        if 1 <= depth <= 3:
            assert far_apart(want[1]).any(), "inputs: values on both sides of -2^36"
        if depth == 4:      # (the maximiser walks into the dead ends: the lowest value is -0.82 * 2^36)
            assert (want[1][legal] < -(1 << 35)).any() and (want[1][legal] > -(1 << 33)).any()
    if case == ("random", 16, 1) and depth == 4:
        assert stats["composed"] >= 2 and stats["anchored"] >= 16 and max(abs(s) for s in sums[-1]) > 1 << 52, "inputs: HUGE at depth 4"
    both_adaptive_forms(g, torch, net, boards, constant(depth), want, [depth] * len(boards), f"{case}, depth {depth}")


MIXED_LAUNCH = (2, 4, 3, 1, 1, 0) + (0,) * 11    # by empty cells: full boards at depth 2, one-empty at 4, two-empty at 3


@pytest.mark.parametrize("case", [("random", 16, 1)], ids=str)
def test_one_adaptive_launch_mixes_the_depths_at_the_value_extremes(g, torch_cuda, case):
    """One launch, every depth: the rows are those the constant schedules and the deep search were checked against."""
    torch = torch_cuda
    rnet = net_of(case)
    net = device_net(g, rnet)
    boards = np.concatenate([DEAD_ENDS, HUGE, SYMMETRIC, MIRRORED, TWO_EMPTY, cleared(HUGE, (0, 5)), cleared(TURNED, (3, 6, 9)),
                             cleared(HUGE, (0, 2, 5, 7)), TURNED])
    depths = np.asarray(MIXED_LAUNCH)[(boards == 0).sum(1)]
    assert depths.tolist() == [2, 2, 4, 4, 3, 3, 3, 1, 1, 0, 4] and set(depths.tolist()) == {0, 1, 2, 3, 4}
    want = (np.zeros(len(boards), np.uint8), np.zeros((len(boards), 4), np.int64))
    for d in range(5):
        at = np.nonzero(depths == d)[0]
        if d == 4:
            at = at[:-1]        # (TURNED at depth 4: the quarter turn of HUGE's row)
        want[0][at], want[1][at] = expected(torch, g, case, boards[at], d)
    want[1][-1] = np.roll(want[1][2], -1)
    want[0][-1] = (int(want[0][2]) - 1) % 4
    assert (TURNED == np.rot90(HUGE.reshape(4, 4)).reshape(1, 16)).all() and ref.move(ref.plain(TURNED[0]), 0)[1] == ref.move(ref.plain(HUGE[0]), 1)[1]
    assert len(set(want[1][2].tolist())) == 4, "inputs: HUGE's four values differ, so the turned action is the turned direction"
    check_ranges(boards[depths > 0], (want[0][depths > 0], want[1][depths > 0]), rnet.frac_bits)
    both_adaptive_forms(g, torch, net, boards, MIXED_LAUNCH, want, depths, "mixed launch")
    # and with every third board masked out
    eng = engine_with(g, boards)
    try:
        m = np.arange(len(boards)) % 3 != 0
        got = adaptive_np(eng.ntuple_adaptive_search(net, MIXED_LAUNCH, active=dev_u32(torch, m)))
        assert_search_equal((got[0][m], got[1][m]), (want[0][m], want[1][m]), boards[m], "mixed launch, masked")
        assert (got[0][~m] == 0).all() and (got[1][~m] == ILLEGAL).all() and got[2].tolist() == np.where(m, depths, 0xff).tolist()
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 3. evaluate and depth 1
@pytest.mark.parametrize("case", UNIFORM + ["staged", "mixed"], ids=str)
def test_evaluate_and_depth_1_on_tiles_of_2_to_the_29(g, torch_cuda, case):
    """test_values_at_the_stated_bounds has tiles of 2^14 .. 2^17; these boards add gains of 2^30 + 2^29 << F."""
    torch = torch_cuda
    rnet = net_of(case)
    net = device_net(g, rnet)
    boards = np.concatenate([BIG, cleared(HUGE, (0, 2, 5, 7))])
    gains = [ref.move(ref.plain(b), d)[1] for b in boards for d in range(4)]
    assert 3 << 29 <= max(gains) < 1 << 31
    want_0, want_1 = reference_rows(boards, 0, rnet), reference_rows(boards, 1, rnet)
    check_ranges(boards, want_1, rnet.frac_bits)
    assert (want_0[1] != ILLEGAL).all(1).any() and (rnet.frac_bits == 0 or (want_1[1] > 1 << 46).any())
    d = dev(torch, boards)
    r = net.evaluate(d)
    assert_search_equal((r.action.cpu().numpy(), r.value.cpu().numpy()), want_0, boards, f"{case}, evaluate")
    assert_search_equal(to_np(net.search(d, 1)), want_1, boards, f"{case}, search depth 1")
    eng = engine_with(g, boards)
    try:
        r = eng.ntuple_evaluate(net)
        assert_search_equal((r.action.cpu().numpy(), r.value.cpu().numpy()), want_0, boards, f"{case}, evaluate, engine")
        assert_search_equal(to_np(eng.ntuple_search(net, 1)), want_1, boards, f"{case}, search depth 1, engine")
    finally:
        eng.close()
