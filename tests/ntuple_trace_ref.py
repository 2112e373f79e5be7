"""Pure-Python reference of the n-tuple traces, TD(lambda) and TC(lambda) (include/g2048.h "N-tuple traces", INTEGRATION.md
§12) -- TEST INFRASTRUCTURE ONLY.

Written from the definition on Python integers.  The one-step updates a trace update is made of are those of
tests/ntuple_ref.py (``update``) and tests/ntuple_tc_ref.py (``tc_update``), called with the list of (afterstate, d_k) pairs
the definition names -- in k-major order, all of phase W before any of phase A.

``push`` and the updates can leave a trace -- a dict of counters of the edges the tests name -- so that a test can show from
the reference alone that its input reaches them:
  push:    "pushes" calls; "wrap" calls whose slot wrapped to 0; "saturate" boards with l + 1 > H (len stays H);
           "ended" boards whose old byte had bit 7 (the flag is consumed: l = 0); "garbage" boards whose old byte's low bits
           exceed H; "term" boards that terminated in this push
  update:  "short" items with k >= L; "clamp_d" boards whose delta was clamped; "zero" boards with d == 0;
           "dk_zero" items with k > 0, d_0 != 0 and d_k == 0; "neg_floor" items with k > 0 and d_k == -1;
           "items" items handed to the one-step update (d_k != 0); plus the counters of the one-step reference
           ("sat", "multi", "rate0", ... ; TD: "zero" also counts zero steps, so read "zero_step" for those)
"""
from __future__ import annotations

import numpy as np

import ntuple_ref as ref
import ntuple_tc_ref as tcref

TRACE_MAX = 8
ONE = 1 << 16
ENDED = 0x80


def _count(trace, key, by=1):
    if trace is not None:
        trace[key] = trace.get(key, 0) + int(by)


def wrap_i64(x):
    return (x + (1 << 63)) % (1 << 64) - (1 << 63)


def push_len(old, H, terminated, trace=None):
    """The len byte push writes for the old byte ``old``."""
    assert 0 <= old <= 255 and 1 <= H <= TRACE_MAX
    low = old & 0x7f
    l = 0 if old & ENDED else min(low, H)
    _count(trace, "ended", bool(old & ENDED))
    _count(trace, "garbage", low > H)
    _count(trace, "saturate", l + 1 > H)
    _count(trace, "term", bool(terminated))
    return min(l + 1, H) | (ENDED if terminated else 0)


def decay(lam, k):
    """p_k in Q16."""
    assert 0 <= lam <= ONE
    p = ONE
    for _ in range(k):
        p = (p * lam) >> 16
    return p


def d_k(delta, lam, k):
    """(clamp(delta) * p_k) >> 16; Python's >> floors."""
    return (tcref.clamp_delta(delta) * decay(lam, k)) >> 16


class Trace:
    """hist uint8 [H, n, 16], len uint8 [n], slot = the slot of the last push (H - 1 before the first)."""

    def __init__(self, n, depth, lam_q16):
        assert 1 <= depth <= TRACE_MAX and 0 <= lam_q16 <= ONE
        self.n, self.depth, self.lam = n, depth, lam_q16
        self.hist = np.zeros((depth, n, 16), np.uint8)
        self.len = np.zeros(n, np.uint8)
        self.slot = depth - 1

    def copy(self):
        t = Trace(self.n, self.depth, self.lam)
        t.hist, t.len, t.slot = self.hist.copy(), self.len.copy(), self.slot
        return t


def push(tr, after, after_value, best_next, terminated, trace=None):
    """Advance the slot and push; returns delta as an int64 array."""
    tr.slot = (tr.slot + 1) % tr.depth
    _count(trace, "pushes")
    _count(trace, "wrap", tr.slot == 0 and trace is not None and trace["pushes"] > 1)
    tr.hist[tr.slot] = np.asarray(after, np.uint8).reshape(tr.n, 16)
    delta = np.zeros(tr.n, np.int64)
    for i in range(tr.n):
        term = bool(terminated[i])
        delta[i] = wrap_i64((0 if term else int(best_next[i])) - int(after_value[i]))
        tr.len[i] = push_len(int(tr.len[i]), tr.depth, term, trace)
    return delta


def items(tr, deltas, trace=None):
    """(boards, d_k) of the work items of an update that have k < L, k-major."""
    H, boards, dks = tr.depth, [], []
    assert len(deltas) == tr.n
    for i in range(tr.n):
        d = tcref.clamp_delta(deltas[i])
        _count(trace, "clamp_d", d != int(deltas[i]))
        _count(trace, "zero", d == 0)
    for k in range(H):
        s = (tr.slot + H - k) % H
        for i in range(tr.n):
            if k >= min(int(tr.len[i]) & 0x7f, H):
                _count(trace, "short")
                continue
            dk = d_k(deltas[i], tr.lam, k)
            if k > 0:
                _count(trace, "dk_zero", dk == 0 and tcref.clamp_delta(deltas[i]) != 0)
                _count(trace, "neg_floor", dk == -1)
            if dk != 0:
                _count(trace, "items")
                boards.append(tr.hist[s, i])
                dks.append(dk)
    return (np.array(boards, np.uint8).reshape(-1, 16), dks)


def trace_update(net, tr, deltas, lr_shift, trace=None):
    """The TD form, in place on net.weights."""
    boards, dks = items(tr, deltas, trace)
    sub = None if trace is None else {}
    ref.update(net, boards, dks, lr_shift, sub)
    if trace is not None:
        _count(trace, "zero_step", sub.get("zero", 0))
        _count(trace, "sat", sub.get("sat", 0))
        _count(trace, "wrap32", sub.get("wrap", 0))


def tc_trace_update(net, tc, tr, deltas, lr_shift, phases=3, trace=None):
    """The TC form, in place on net.weights (phase W) and tc.err / tc.mag (phase A)."""
    boards, dks = items(tr, deltas, trace)
    sub = None if trace is None else {}
    tcref.tc_update(net, tc, boards, dks, lr_shift, phases, sub)
    if trace is not None:
        for key, v in sub.items():
            if key not in ("zero", "clamp_d"):
                _count(trace, key, v)


# ------------------------------------------------------------------------------ the TD form on whole arrays (replays)
def offsets_np(boards, net):
    """int64 [8, T, n]: idx_t(s(board_i)) for every symmetry, tuple and board, by the permutations of ntuple_ref."""
    b = np.asarray(boards, np.int64).reshape(-1, 16) % 32
    c = np.minimum(b, 15)
    out = np.zeros((8, len(net.tuples), len(c)), np.int64)
    for s, perm in enumerate(ref._sym_perms()):
        sb = c[:, list(perm)]                              # symmetries(): s(b)[k] = b[perm[k]]
        for t, cells in enumerate(net.tuples):
            for k, cell in enumerate(cells):
                out[s, t] |= sb[:, cell] << (4 * k)
    return out


def trace_update_np(net, tr, deltas, lr_shift):
    """``trace_update`` with numpy arithmetic on whole arrays -- for replays of many steps.  tests/test_ntuple_trace_host.py
    pins it to the scalar version above."""
    H = tr.depth
    d = np.clip(np.asarray(deltas, np.int64), -tcref.MAX_DELTA, tcref.MAX_DELTA)
    L = np.minimum(tr.len & 0x7f, H)
    w = net.weights                                        # int64 holding int32 values: sums of steps cannot overflow it
    for k in range(H):
        dk = (d * decay(tr.lam, k)) >> 16                  # |d * p_k| <= 2^56; numpy's >> on int64 is arithmetic
        step = np.clip(dk >> lr_shift, ref.INT32_MIN, ref.INT32_MAX)
        step[k >= L] = 0
        live = np.nonzero(step)[0]
        if len(live) == 0:
            continue
        off = offsets_np(tr.hist[(tr.slot + H - k) % H][live], net)
        for s in range(8):
            for t in range(len(net.tuples)):
                np.add.at(w[t], off[s, t], step[live])
    net.weights[:] = (w + (1 << 31)) % (1 << 32) - (1 << 31)
