"""Pure-Python reference of the n-tuple delay, delayed TD(lambda) and TC(lambda) (include/g2048.h "N-tuple delay",
INTEGRATION.md §19) -- TEST INFRASTRUCTURE ONLY.

Written from the definition on Python integers, in two independent forms:

* the ring model -- ``Delay``, ``push``, ``due_items`` and the two updates: the trace ring of tests/ntuple_trace_ref.py plus an
  accumulator per slot and board; an update hands the (afterstate, D) pairs that are due to the one-step references
  (tests/ntuple_ref.py, tests/ntuple_tc_ref.py, tests/ntuple_staged_ref.py for a network with thresholds), k-major, all of
  phase W before any of phase A;
* the closed form of consequence 1 -- ``closed_totals``: for the afterstate pushed at step t, the sum over k = 0..m of
  ``(clamp(delta_{t+k}) * p_k) >> 16`` with m ending at H - 1, at the first push that terminated, or at the last push.  It
  knows nothing of slots, len bytes or modes.

``applied_totals`` runs the ring model over a sequence of pushes, a STEP update after each and one FLUSH, and returns what
every pushed afterstate was applied with and how often; tests/test_ntuple_delay_cpu.py compares it with ``closed_totals``.
"""
from __future__ import annotations

import numpy as np

import ntuple_ref as ref
import ntuple_staged_ref as sref
import ntuple_tc_ref as tcref
import ntuple_trace_ref as tref

STEP, FLUSH = 0, 1
ENDED = tref.ENDED


class Delay(tref.Trace):
    """The trace ring plus acc, a [H][n] list of Python ints (|acc| <= 2^43)."""

    def __init__(self, n, depth, lam_q16):
        super().__init__(n, depth, lam_q16)
        self.acc = [[0] * n for _ in range(depth)]

    def copy(self):
        d = Delay(self.n, self.depth, self.lam)
        d.hist, d.len, d.slot = self.hist.copy(), self.len.copy(), self.slot
        d.acc = [row[:] for row in self.acc]
        return d

    def acc_i64(self):
        return np.array(self.acc, np.int64).reshape(self.depth, self.n)


def kept(old, H):
    """l of push: the valid slots an old len byte stands for."""
    return 0 if old & ENDED else min(old & 0x7f, H)


def push(dl, after, after_value, best_next, terminated, trace=None):
    """Advance the slot and push; returns delta as an int64 array."""
    H, old = dl.depth, [int(x) for x in dl.len]
    delta = tref.push(dl, after, after_value, best_next, terminated, trace)   # slot, hist, delta, len: exactly the trace push
    for i in range(dl.n):
        L = min(kept(old[i], H) + 1, H)
        d = tcref.clamp_delta(int(delta[i]))
        dl.acc[dl.slot][i] = d
        for k in range(1, L):
            dl.acc[(dl.slot + H - k) % H][i] += (d * tref.decay(dl.lam, k)) >> 16
    return delta


def is_due(len_byte, k, H, mode):
    """Whether item (k, i) applies something in this mode; None for an item that does not exist (k >= L)."""
    if k >= min(len_byte & 0x7f, H):
        return None
    ended = bool(len_byte & ENDED)
    return (ended or k == H - 1) if mode == STEP else (not ended and k != H - 1)


def due_items(dl, mode, order=None):
    """(boards uint8 [m, 16], D list) of the due items, k-major (or in ``order``, a sequence of item numbers k * n + i); D is
    clamped, and zero D are kept (the one-step references skip them)."""
    assert mode in (STEP, FLUSH)
    H, boards, Ds = dl.depth, [], []
    for item in (range(H * dl.n) if order is None else order):
        k, i = divmod(item, dl.n)
        if is_due(int(dl.len[i]), k, H, mode):
            s = (dl.slot + H - k) % H
            boards.append(dl.hist[s, i])
            Ds.append(tcref.clamp_delta(dl.acc[s][i]))
    return np.array(boards, np.uint8).reshape(-1, 16), Ds


def _staged(net):
    return getattr(net, "thr", None) is not None


def delay_update(net, dl, lr_shift, mode=STEP, order=None):
    """The TD form, in place on net.weights (an ntuple_ref.Net, or an ntuple_staged_ref.StagedNet)."""
    boards, Ds = due_items(dl, mode, order)
    (sref if _staged(net) else ref).update(net, boards, Ds, lr_shift)


def tc_delay_update(net, tc, dl, lr_shift, phases=3, mode=STEP, order=None):
    """The TC form, in place on net.weights (phase W) and tc.err / tc.mag (phase A)."""
    boards, Ds = due_items(dl, mode, order)
    (sref if _staged(net) else tcref).tc_update(net, tc, boards, Ds, lr_shift, phases)


# ------------------------------------------------------------------------------------------------ consequence 1, two ways
def closed_totals(deltas, terms, H, lam):
    """{(t, i): total} from the closed form alone.  deltas[t][i], terms[t][i] for pushes t = 0..P-1."""
    P, out = len(deltas), {}
    for t in range(P):
        for i in range(len(deltas[t])):
            total, k = 0, 0
            while True:
                total += (tcref.clamp_delta(int(deltas[t + k][i])) * tref.decay(lam, k)) >> 16
                if k == H - 1 or terms[t + k][i] or t + k == P - 1:
                    break
                k += 1
            out[(t, i)] = total
    return out


def applied_totals(deltas, terms, H, lam, flush=True, start_len=None):
    """The ring model over the same pushes, a STEP update after each and (``flush``) one FLUSH at the end:
    {(t, i): [the accumulator of every time the afterstate pushed at t was due]} -- exactly one entry each, if consequence 1
    holds.  The pushes carry no boards: the slot's tag says which push filled it."""
    n = len(deltas[0])
    dl = Delay(n, H, lam)
    if start_len is not None:
        dl.len[:] = start_len
    tag = [[None] * n for _ in range(H)]
    out = {}

    def apply(mode):
        for k in range(H):
            for i in range(n):
                if is_due(int(dl.len[i]), k, H, mode):
                    s = (dl.slot + H - k) % H
                    out.setdefault((tag[s][i], i), []).append(dl.acc[s][i])

    zeros = np.zeros((n, 16), np.uint8)
    for t in range(len(deltas)):
        # after_value = 0 and best_next = delta make push form exactly deltas[t]; a terminated board's delta is -after_value
        term = np.array([bool(x) for x in terms[t]])
        d = np.array([int(x) for x in deltas[t]], dtype=object)
        av = np.array([-int(x) if tm else 0 for x, tm in zip(d, term)], dtype=object)
        best = np.array([0 if tm else int(x) for x, tm in zip(d, term)], dtype=object)
        got = push(dl, zeros, av, best, term)
        assert [int(x) for x in got] == [tref.wrap_i64(int(x)) for x in d]
        for i in range(n):
            tag[dl.slot][i] = t
        apply(STEP)
    if flush:
        apply(FLUSH)
    return out
