"""Pure-Python reference of temporal-coherence learning for the n-tuple network (include/g2048.h "Temporal-coherence (TC)
learning") -- TEST INFRASTRUCTURE ONLY.

Written from the definition on Python integers (no numpy arithmetic in ``rate`` / ``step``); moves, symmetries, indices
and evaluate are those of tests/ntuple_ref.py.  The tables only store: ``err`` is an int64 array, ``mag`` a uint64 array (the
unsigned reading of the device's int64); every entry is turned into a Python int before it is used.

``tc_update`` can leave a trace -- a dict of counters of the edges the tests name -- so that a test can show from the
reference alone that its input reaches them:
  "k"        look-ups whose A needs a shift (bitlen(A) > 32)          "rate0" / "rate1"  look-ups with rate 0 / 65 536
  "clamp_m"  look-ups with |E| > A (m clamped to A)                   "clamp_d"          boards whose delta was clamped
  "sat"      look-ups whose step saturated                            "zero"             boards with d == 0 (untouched)
  "zero_step" look-ups with d != 0 whose step is 0                    "multi"            entries hit more than once in the call
"""
from __future__ import annotations

import numpy as np

import ntuple_ref as ref

ONE = 1 << 16
MAX_DELTA = 1 << 40
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
M64 = (1 << 64) - 1


def rate(E, A, trace=None):
    """rate(E, A) in Q16 for E a signed and A an unsigned 64-bit integer."""
    assert INT64_MIN <= E <= INT64_MAX and 0 <= A <= M64
    if A == 0:
        r = ONE
    else:
        m = min(abs(E), A)
        k = max(0, A.bit_length() - 32)
        r = ((m >> k) << 16) // (A >> k)
        if trace is not None:
            trace["k"] = trace.get("k", 0) + (k > 0)
            trace["clamp_m"] = trace.get("clamp_m", 0) + (abs(E) > A)
    if trace is not None:
        trace["rate0"] = trace.get("rate0", 0) + (r == 0)
        trace["rate1"] = trace.get("rate1", 0) + (r == ONE)
    return r


def clamp_delta(delta):
    return max(-MAX_DELTA, min(MAX_DELTA, int(delta)))


def step(delta, r, lr_shift, trace=None):
    """sat_int32((clamp(delta) * r) >> (16 + lr_shift)); Python's >> floors."""
    x = (clamp_delta(delta) * r) >> (16 + lr_shift)
    s = max(ref.INT32_MIN, min(ref.INT32_MAX, x))
    if trace is not None:
        trace["sat"] = trace.get("sat", 0) + (s != x)
    return s


class Sparse(dict):
    """A table [T, 16^L] of zeros that stores only the entries written: for shapes too wide to hold on the host."""

    def __init__(self, shape):
        super().__init__()
        self.shape = shape

    def __missing__(self, key):
        return 0


class TC:
    """err: int64 [T, 16^L]; mag: uint64 [T, 16^L] (the unsigned reading of the device's int64) -- or ``Sparse`` tables."""

    def __init__(self, net, err=None, mag=None):
        self.err = np.zeros(net.weights.shape, np.int64) if err is None else err
        self.mag = np.zeros(net.weights.shape, np.uint64) if mag is None else mag

    def copy(self):
        return TC(None, self.err.copy(), self.mag.copy())

    def mag_i64(self):
        """mag as the int64 bit pattern the device holds."""
        return self.mag.view(np.int64)


def sparse_net(tuples, frac_bits=10):
    """(ntuple_ref.Net, TC) with Sparse tables, all zero."""
    net = ref.Net.__new__(ref.Net)
    net.tuples, net.frac_bits = [tuple(t) for t in tuples], frac_bits
    shape = (len(net.tuples), 16 ** len(net.tuples[0]))
    net.weights = Sparse(shape)
    return net, TC(None, Sparse(shape), Sparse(shape))


def wrap_i64(x):
    return (x + (1 << 63)) % (1 << 64) - (1 << 63)


def hits_of(board, net):
    """The (t, idx) of the 8T look-ups of one board, in the order of ntuple_ref.value."""
    out = []
    ref.value(ref.plain(board), net, out)
    return out


def tc_update(net, tc, boards, deltas, lr_shift, phases=3, trace=None):
    """In place on net.weights (phase W, bit 1) and tc.err / tc.mag (phase A, bit 2).  Phase W reads the accumulators as
    they are before the call: it runs to its end before phase A starts."""
    assert phases in (1, 2, 3) and 0 <= lr_shift <= 40
    boards = np.asarray(boards).reshape(-1, 16)
    work = []
    for b, delta in zip(boards, deltas):
        d = clamp_delta(delta)
        if trace is not None:
            trace["clamp_d"] = trace.get("clamp_d", 0) + (d != int(delta))
            trace["zero"] = trace.get("zero", 0) + (d == 0)
        if d != 0:
            work.append((hits_of(b, net), d))
    if trace is not None:
        seen = {}
        for hits, _ in work:
            for h in hits:
                seen[h] = seen.get(h, 0) + 1
        trace["multi"] = trace.get("multi", 0) + sum(1 for c in seen.values() if c > 1)
    if phases & 1:
        for hits, d in work:
            for t, i in hits:
                s = step(d, rate(int(tc.err[t, i]), int(tc.mag[t, i]), trace), lr_shift, trace)
                if trace is not None:
                    trace["zero_step"] = trace.get("zero_step", 0) + (s == 0)
                net.weights[t, i] = ref.wrap32(int(net.weights[t, i]) + s)
    if phases & 2:
        for hits, d in work:
            for t, i in hits:
                tc.err[t, i] = wrap_i64(int(tc.err[t, i]) + d)
                tc.mag[t, i] = (int(tc.mag[t, i]) + abs(d)) & M64


def tc_step(envs, net, tc, lr_shift, trace=None):
    """ntuple_ref.td_step with the TC update in place of the TD(0) one.  ``trace["episodes"]`` counts the episodes that
    ended."""
    first = [ref.evaluate(ref.env_board(e), net) for e in envs]
    terminated = []
    for e, (_, action, *_rest) in zip(envs, first):
        _, term, _, _ = e.step(action)
        if term:
            e.reset()
        terminated.append(term)
    second = [ref.evaluate(ref.env_board(e), net) for e in envs]
    deltas = [(0 if term else s[2]) - f[4] for f, s, term in zip(first, second, terminated)]
    tc_update(net, tc, [f[3] for f in first], deltas, lr_shift, 3, trace)
    if trace is not None:
        trace["episodes"] = trace.get("episodes", 0) + sum(terminated)
