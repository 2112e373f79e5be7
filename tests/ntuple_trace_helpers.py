"""Shared by the n-tuple trace tests: synthetic push sequences whose termination masks make the ring wrap, fill and clear,
and deltas (the host build is ntuple_helpers').  A plain module, like ntuple_tc_helpers."""
import numpy as np

from analysis_helpers import mixed_boards

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


def push_inputs(n, pushes, seed, span=1 << 30):
    """``pushes`` synthetic pushes of n boards: a list of (after uint8 [n, 16], after_value, best_next int64 [n], terminated
    uint8 [n]).  Board i terminates at push t when (t + i) % (i % 5 + 3) == 0 -- every board ends several times in twelve
    pushes, at different phases, and board 2 (period 5) has runs of four pushes without an end -- except boards with
    i % 7 == 6, which never end.  Non-zero bytes of ``terminated`` are 1, 2 or 0xff."""
    rng = np.random.default_rng(seed)
    boards = mixed_boards(n * pushes, seed).reshape(pushes, n, 16)
    out = []
    for t in range(pushes):
        i = np.arange(n)
        term = (((t + i) % (i % 5 + 3) == 0) & (i % 7 != 6)).astype(np.uint8) * np.array([1, 2, 0xff], np.uint8)[(t + i) % 3]
        out.append((boards[t], rng.integers(-span, span, n), rng.integers(-span, span, n), term))
    return out


def trace_deltas(n, seed):
    """Mixed-sign deltas for a trace update: small ones whose d_k reaches 0 or sticks at -1, sizes up to beyond the clamp,
    zeros, and the int64 extremes."""
    rng = np.random.default_rng(seed)
    d = rng.integers(-(1 << 20), 1 << 20, n) << rng.integers(0, 22, n)
    d[::9] = 0
    special = [3, -3, 1, -1, (1 << 40) + 1, -(1 << 40) - 1, INT64_MAX, INT64_MIN, 1 << 40, -(1 << 40), 1 << 31, -(1 << 31) - 1, 2, -2]
    d[1::4][:len(special)] = special[:len(d[1::4])]
    return d
