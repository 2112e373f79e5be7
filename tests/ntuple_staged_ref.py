"""Pure-Python reference of the multi-stage n-tuple network (include/g2048.h "Multi-stage n-tuple networks", INTEGRATION.md
§13) -- TEST INFRASTRUCTURE ONLY.

Written from the definition on top of tests/ntuple_ref.py, ntuple_tc_ref.py, ntuple_trace_ref.py and ntuple_search_ref.py and
nothing from the device header: ``mask`` and ``stage`` are the two formulas on Python integers, a ``StagedNet`` holds
``weights [S, T, 16^L]`` and ``sub(s)`` is an ``ntuple_ref.Net`` that views ``weights[s]`` in place -- so V, the update, the TC
phases and the trace items ARE the existing reference functions, called on ``sub(stage(board))``.  Evaluate and search have
thin versions of their own because the stage is chosen per afterstate and per leaf.

The functions can leave a trace -- a dict of counters of the edges the tests name -- so that a test can show from the
reference alone that its input reaches them:
  "stage"        {s: boards (of values / update / stage_batch) or afterstates and leaves (of evaluate / search) in stage s}
  "after_span"   boards whose legal afterstates lie in at least 2 stages (evaluate)
  "chance_span"  chance nodes whose children lie in at least 2 stages (search)
  "leaf_other"   leaves (depth-0 afterstates) of a search in another stage than the root board
  "hist_span"    boards whose live trace slots lie in at least 2 stages (trace updates)
  "at_thr" / "below_thr"   boards whose mask equals a threshold / is exactly one below a threshold
"""
from __future__ import annotations

import numpy as np

import ntuple_ref as ref
import ntuple_search_ref as sref
import ntuple_tc_ref as tcref
import ntuple_trace_ref as tref

MAX_STAGES = 8
ILLEGAL = ref.ILLEGAL


def mask(b):
    """OR over the 16 cells of 1 << c(cell): bit 0 is "has an empty cell"."""
    m = 0
    for e in b:
        m |= 1 << ref.cell(int(e))
    return m


def stage(b, thr, trace=None):
    """The number of thresholds mask(b) is not below."""
    m = mask(b)
    s = sum(1 for t in thr if m >= t)
    if trace is not None:
        trace.setdefault("stage", {})
        trace["stage"][s] = trace["stage"].get(s, 0) + 1
        trace["at_thr"] = trace.get("at_thr", 0) + (m in thr)
        trace["below_thr"] = trace.get("below_thr", 0) + (m + 1 in thr)
    return s


def stage_mask(*tiles):
    m = 0
    for t in tiles:
        m |= 1 << min(int(t).bit_length() - 1, 15)
    return m


def _view(tuples, frac_bits, weights):
    net = ref.Net.__new__(ref.Net)
    net.tuples, net.frac_bits, net.weights = tuples, frac_bits, weights
    return net


class StagedNet:
    """tuples, frac_bits as ntuple_ref.Net; thr: the S - 1 ascending thresholds; weights: int64 [S, T, 16^L] holding int32
    values (or a list of S ``ntuple_tc_ref.Sparse`` tables)."""

    def __init__(self, tuples, thr, frac_bits=10, weights=None):
        self.tuples = [tuple(t) for t in tuples]
        self.thr = tuple(int(t) for t in thr)
        assert len(self.thr) < MAX_STAGES and all(1 <= t <= 65535 for t in self.thr)
        assert all(a < b for a, b in zip(self.thr, self.thr[1:]))
        self.frac_bits = frac_bits
        shape = (len(self.thr) + 1, len(self.tuples), 16 ** len(self.tuples[0]))
        self.weights = np.zeros(shape, np.int64) if weights is None else weights

    @property
    def n_stages(self):
        return len(self.thr) + 1

    def copy(self):
        return StagedNet(self.tuples, self.thr, self.frac_bits, self.weights.copy())

    def sub(self, s):
        """An ntuple_ref.Net on weights[s], in place."""
        return _view(self.tuples, self.frac_bits, self.weights[s])

    def of(self, b, trace=None):
        return self.sub(stage(b, self.thr, trace))


def sparse_net(tuples, thr, frac_bits=10):
    """A StagedNet whose S tables are ntuple_tc_ref.Sparse: for shapes too wide to hold on the host."""
    shape = (len(tuples), 16 ** len(tuples[0]))
    return StagedNet(tuples, thr, frac_bits, [tcref.Sparse(shape) for _ in range(len(thr) + 1)])


class StagedTC:
    """err int64, mag uint64, both [S, T, 16^L]; sub(s) is an ntuple_tc_ref.TC on the tables of stage s, in place."""

    def __init__(self, net, err=None, mag=None):
        self.err = np.zeros(net.weights.shape, np.int64) if err is None else err
        self.mag = np.zeros(net.weights.shape, np.uint64) if mag is None else mag

    def copy(self):
        return StagedTC(None, self.err.copy(), self.mag.copy())

    def sub(self, s):
        return tcref.TC(None, self.err[s], self.mag[s])

    def mag_i64(self):
        return self.mag.view(np.int64)


def random_net(tuples, thr, seed, frac_bits=10, lo=-(1 << 31), hi=1 << 31):
    """A StagedNet with a different uniform table in [lo, hi) per stage."""
    net = StagedNet(tuples, thr, frac_bits)
    net.weights[:] = np.random.default_rng(seed).integers(lo, hi, size=net.weights.shape)
    return net


def stage_batch(boards, thr, trace=None):
    return np.array([stage(ref.plain(b), thr, trace) for b in np.asarray(boards).reshape(-1, 16)], np.uint8)


def value(b, net, trace=None):
    """V(b), from the tables of stage(b)."""
    return ref.value(b, net.of(b, trace))


def values_batch(boards, net, trace=None):
    return np.array([value(ref.plain(b), net, trace) for b in np.asarray(boards).reshape(-1, 16)], np.int64)


def evaluate(board, net, trace=None):
    """ntuple_ref.evaluate with V of every afterstate read from the afterstate's own stage."""
    b = ref.plain(board)
    q, after, vals, stages = [ILLEGAL] * 4, [b] * 4, [0] * 4, set()
    for d in range(4):
        a, g, legal = ref.move(b, d)
        if legal:
            stages.add(stage(a, net.thr))
            vals[d] = value(a, net, trace)
            q[d] = (g << net.frac_bits) + vals[d]
            after[d] = a
    if trace is not None:
        trace["after_span"] = trace.get("after_span", 0) + (len(stages) > 1)
    legal = [d for d in range(4) if q[d] != ILLEGAL]
    if not legal:
        return q, 0, 0, b, 0
    action = max(legal, key=lambda d: (q[d], -d))
    return q, action, q[action], after[action], vals[action]


def evaluate_batch(boards, net, trace=None):
    """(value int64 [n, 4], action uint8 [n], best int64 [n], after uint8 [n, 16], after_value int64 [n])."""
    boards = np.asarray(boards).reshape(-1, 16)
    n = len(boards)
    val, act = np.zeros((n, 4), np.int64), np.zeros(n, np.uint8)
    best, after, av = np.zeros(n, np.int64), np.zeros((n, 16), np.uint8), np.zeros(n, np.int64)
    for i, b in enumerate(boards):
        q, act[i], best[i], a, av[i] = evaluate(b, net, trace)
        val[i] = q
        after[i] = a
    return val, act, best, after, av


# ------------------------------------------------------------------------------------------------ search
def after_value(a, k, net, trace=None, root_stage=None):
    """A_k(a) of ntuple_search_ref with the staged V at the leaves."""
    if k == 0:
        if trace is not None and root_stage is not None:
            trace["leaf_other"] = trace.get("leaf_other", 0) + (stage(a, net.thr) != root_stage)
        return value(a, net, trace)
    empty = [c for c in range(16) if a[c] == 0]
    total, stages = 0, set()
    for c in empty:
        for exponent, weight in ((1, 9), (2, 1)):
            child = a[:c] + (exponent,) + a[c + 1:]
            stages.add(stage(child, net.thr))
            total += weight * state_value(child, k - 1, net, trace, root_stage)
    if trace is not None:
        trace["chance"] = trace.get("chance", 0) + 1
        trace["chance_span"] = trace.get("chance_span", 0) + (len(stages) > 1)
    return total // (10 * len(empty))


def state_value(b, k, net, trace=None, root_stage=None):
    """S_k(b).  ``trace["memo"]``, when the caller puts a dict there, remembers S_k of boards already searched below the same
    root stage (a depth-2 tree reaches the same child along many paths); the counters then count each such board once."""
    memo = None if trace is None else trace.get("memo")
    if memo is not None and (b, k, root_stage) in memo:
        return memo[b, k, root_stage]
    best = _state_value(b, k, net, trace, root_stage)
    if memo is not None:
        memo[b, k, root_stage] = best
    return best


def _state_value(b, k, net, trace, root_stage):
    best = None
    for d in range(4):
        a, g, legal = ref.move(b, d)
        if legal:
            q = (g << net.frac_bits) + after_value(a, k, net, trace, root_stage)
            best = q if best is None or q > best else best
    return 0 if best is None else best


def search(board, depth, net, trace=None):
    """(value[4], action) of one board."""
    b = ref.plain(board)
    root = stage(b, net.thr)
    val = [ILLEGAL] * 4
    for d in range(4):
        a, g, legal = ref.move(b, d)
        if legal:
            val[d] = (g << net.frac_bits) + after_value(a, depth, net, trace, root)
    legal = [d for d in range(4) if val[d] != ILLEGAL]
    if not legal:
        return val, 0
    return val, max(legal, key=lambda d: (val[d], -d))


def search_batch(boards, depth, net, trace=None):
    """(action uint8 [n], value int64 [n, 4])."""
    boards = np.asarray(boards).reshape(-1, 16)
    act, val = np.zeros(len(boards), np.uint8), np.zeros((len(boards), 4), np.int64)
    for i, b in enumerate(boards):
        val[i], act[i] = search(b, depth, net, trace)
    return act, val


# ------------------------------------------------------------------------------------------------ updates
def _by_stage(boards, deltas, thr, trace=None):
    """{s: (boards, deltas) of the boards in stage s}, the order within a stage kept."""
    out = {}
    for b, d in zip(np.asarray(boards).reshape(-1, 16), deltas):
        bs, ds = out.setdefault(stage(ref.plain(b), thr, trace), ([], []))
        bs.append(b)
        ds.append(int(d))
    return out


def update(net, boards, deltas, lr_shift, trace=None):
    """ntuple_ref.update of every board on the tables of its stage, in place."""
    for s, (bs, ds) in _by_stage(boards, deltas, net.thr, trace).items():
        ref.update(net.sub(s), np.array(bs, np.uint8), ds, lr_shift)


def tc_update(net, tc, boards, deltas, lr_shift, phases=3, trace=None):
    """ntuple_tc_ref.tc_update per stage: phase W of every stage before phase A of any (the stages' tables are disjoint, so
    the order of the stages does not matter)."""
    groups = _by_stage(boards, deltas, net.thr, trace)
    for p in (1, 2):
        if phases & p:
            for s, (bs, ds) in groups.items():
                tcref.tc_update(net.sub(s), tc.sub(s), np.array(bs, np.uint8), ds, lr_shift, p)


def _items(net, tr, deltas, trace):
    boards, dks = tref.items(tr, deltas)
    if trace is not None:
        H = tr.depth
        for i in range(tr.n):
            L = min(int(tr.len[i]) & 0x7f, H)
            stages = {stage(ref.plain(tr.hist[(tr.slot + H - k) % H, i]), net.thr) for k in range(L)}
            trace["hist_span"] = trace.get("hist_span", 0) + (len(stages) > 1)
    return boards, dks


def trace_update(net, tr, deltas, lr_shift, trace=None):
    """The TD trace update: the items of ntuple_trace_ref, each on the tables of its afterstate's stage."""
    boards, dks = _items(net, tr, deltas, trace)
    update(net, boards, dks, lr_shift, trace)


def tc_trace_update(net, tc, tr, deltas, lr_shift, phases=3, trace=None):
    boards, dks = _items(net, tr, deltas, trace)
    tc_update(net, tc, boards, dks, lr_shift, phases, trace)


# ------------------------------------------------------------------------------------------------ trainers
def _play(envs, net, trace=None):
    """Points 1-3 of the TD(0) step (ntuple_ref.td_step) with the staged evaluate: (afterstates, after values, best of the
    next boards, terminated)."""
    first = [evaluate(ref.env_board(e), net, trace) for e in envs]
    terminated = []
    for e, (_, action, *_rest) in zip(envs, first):
        _, term, _, _ = e.step(action)
        if term:
            e.reset()
        terminated.append(term)
    second = [evaluate(ref.env_board(e), net) for e in envs]
    return [f[3] for f in first], [f[4] for f in first], [s[2] for s in second], terminated


def td_step(envs, net, lr_shift, trace=None):
    after, av, best, terminated = _play(envs, net, trace)
    deltas = [(0 if term else b) - v for b, v, term in zip(best, av, terminated)]
    update(net, after, deltas, lr_shift)


def tcl_step(envs, net, tc, tr, lr_shift, trace=None):
    """The TC(lambda) step: play, push, then the staged TC trace update."""
    after, av, best, terminated = _play(envs, net, trace)
    deltas = tref.push(tr, np.array(after, np.uint8), av, best, terminated)
    tc_trace_update(net, tc, tr, deltas, lr_shift, 3, trace)
