"""Pure-Python reference of the batch-mean n-tuple update (include/g2048.h "Batch-mean update") -- TEST
INFRASTRUCTURE ONLY.

Written from the definition on Python integers with explicit wraps; moves, symmetries, indices, stages and trace items are those
of tests/ntuple_ref.py, ntuple_staged_ref.py and ntuple_trace_ref.py, imported and not edited.  It works on an
``ntuple_staged_ref.StagedNet`` (``weights [S, T, 16^Lmax]``; ``ntuple_mixed_ref.mixed_net`` builds one for every kind of network,
S = 1 and no thresholds for a network of one weight set) and a ``Mean`` of the same shape, in place.  The items of a call can be
run in any ``order`` (a permutation of the item numbers): the definition says the result does not depend on it.

``mean_update`` can leave a trace -- a dict of the edges the tests name -- so that a test can show from the reference alone that
its input reaches them:
  "zero"       items with d == 0 (untouched)                      "clamp_d"    items whose delta was clamped
  "entries"    distinct entries reached                           "multi"      entries reached by at least 2 different items
  "sym"        entries reached at least twice by ONE item         "max_count"  the largest count of an entry
  "by_table"   {(stage, t): the largest count in that table}      "neg_rem"    entries with sum < 0 that count does not divide
  "cancel"     entries with count >= 2 and sum == 0               "zero_step"  entries whose mean is not 0 and whose step is 0
  "sat"        entries whose step saturated                       "moved"      entries whose weight changed
"""
from __future__ import annotations

import numpy as np

import ntuple_ref as ref
import ntuple_staged_ref as sref
import ntuple_tc_ref as tcref
import ntuple_trace_ref as tref

SUM, APPLY = 1, 2
M32 = (1 << 32) - 1
MAX_ITEMS = 1 << 29


class Mean:
    """sum: int64, count: uint32, both of the shape of the network's weights; zero between calls."""

    def __init__(self, net, sum=None, count=None):
        self.sum = np.zeros(net.weights.shape, np.int64) if sum is None else sum
        self.count = np.zeros(net.weights.shape, np.uint32) if count is None else count

    def copy(self):
        return Mean(None, self.sum.copy(), self.count.copy())

    def is_zero(self):
        return not self.sum.any() and not self.count.any()


def floor_div(a, c):
    """floor(a / c) for c >= 1: Python's // floors."""
    assert c >= 1
    return a // c


def hits_of(board, net):
    """The (stage, t, idx) of the 8T look-ups of one board, in the order of ntuple_ref.value."""
    b = ref.plain(board)
    s, out = sref.stage(b, net.thr), []
    ref.value(b, net.sub(0), out)
    return [(s, t, i) for t, i in out]


def work_of(net, boards, deltas, trace=None):
    """[(hits, d)] of the items that do something: d = clamp(delta) != 0."""
    work = []
    for b, delta in zip(np.asarray(boards).reshape(-1, 16), deltas):
        d = tcref.clamp_delta(delta)
        if trace is not None:
            trace["clamp_d"] = trace.get("clamp_d", 0) + (d != int(delta))
            trace["zero"] = trace.get("zero", 0) + (d == 0)
        if d != 0:
            work.append((hits_of(b, net), d))
    return work


def _reached(work, trace):
    items, most = {}, {}
    for n, (hits, _) in enumerate(work):
        for h in hits:
            items.setdefault(h, []).append(n)
    for h, who in items.items():
        most[h[:2]] = max(most.get(h[:2], 0), len(who))
    trace["entries"] = trace.get("entries", 0) + len(items)
    trace["multi"] = trace.get("multi", 0) + sum(1 for who in items.values() if len(set(who)) > 1)
    trace["sym"] = trace.get("sym", 0) + sum(1 for who in items.values() if len(set(who)) < len(who))
    trace["max_count"] = max(trace.get("max_count", 0), max((len(who) for who in items.values()), default=0))
    by = trace.setdefault("by_table", {})
    for k, v in most.items():
        by[k] = max(by.get(k, 0), v)


def phase_sum(mean, work):
    for hits, d in work:
        for h in hits:
            mean.sum[h] = tcref.wrap_i64(int(mean.sum[h]) + d)
            mean.count[h] = (int(mean.count[h]) + 1) & M32


def phase_apply(net, mean, work, lr_shift, trace=None):
    for hits, _ in work:
        for h in hits:
            c = int(mean.count[h])
            mean.count[h] = 0
            if c == 0:
                continue                                  # another reach of this entry owned it
            a = int(mean.sum[h])
            mean.sum[h] = 0
            m = floor_div(a, c)
            step = ref.step_of(m, lr_shift)
            if trace is not None:
                trace["neg_rem"] = trace.get("neg_rem", 0) + (a < 0 and a % c != 0)
                trace["cancel"] = trace.get("cancel", 0) + (c >= 2 and a == 0)
                trace["zero_step"] = trace.get("zero_step", 0) + (m != 0 and step == 0)
                trace["sat"] = trace.get("sat", 0) + (step != m >> lr_shift)
                trace["moved"] = trace.get("moved", 0) + (step != 0)
            net.weights[h] = ref.wrap32(int(net.weights[h]) + step)


def mean_update(net, mean, boards, deltas, lr_shift, phases=3, trace=None, order=None):
    """In place on mean.sum / mean.count (phase SUM, bit 1) and on all three arrays (phase APPLY, bit 2).  ``order``: the items
    in that order, in both phases."""
    assert phases in (1, 2, 3) and 0 <= lr_shift <= 40
    boards = np.asarray(boards).reshape(-1, 16)
    assert len(boards) == len(deltas) < MAX_ITEMS
    work = work_of(net, boards, deltas, trace)
    if order is not None:
        kept = [i for i, delta in enumerate(deltas) if tcref.clamp_delta(delta) != 0]
        at = {i: w for i, w in zip(kept, work)}
        work = [at[i] for i in order if i in at]
        assert len(work) == len(at)
    if trace is not None:
        _reached(work, trace)
    if phases & SUM:
        phase_sum(mean, work)
    if phases & APPLY:
        phase_apply(net, mean, work, lr_shift, trace)


def mean_trace_update(net, mean, tr, deltas, lr_shift, phases=3, trace=None, order=None):
    """The items (afterstate, d_k) of ntuple_trace_ref, through mean_update: |d_k| <= 2^40, so its clamp changes nothing."""
    boards, dks = tref.items(tr, deltas)
    if len(dks):
        mean_update(net, mean, boards, dks, lr_shift, phases, trace, order)


def mean_step(envs, net, mean, lr_shift, trace=None):
    """ntuple_staged_ref.td_step with the batch-mean update in place of the summed one."""
    after, av, best, terminated = sref._play(envs, net)
    deltas = [(0 if term else b) - v for b, v, term in zip(best, av, terminated)]
    mean_update(net, mean, after, deltas, lr_shift, 3, trace)
    return np.array(after, np.uint8), np.array(deltas, np.int64)
