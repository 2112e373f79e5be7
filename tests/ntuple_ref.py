"""Pure-Python / numpy reference of the n-tuple network value function (include/g2048.h "N-tuple network",
INTEGRATION.md §9) -- TEST INFRASTRUCTURE ONLY.

Written from the definition with nothing from the device header: a move slides four lines through ``shift_row`` (the
game's rule written out cell by cell; tests/test_ntuple_host.py pins it to the oracle's row table), the eight symmetries
are numpy's ``flip`` and ``rot90`` exactly as ``training_data.augment()`` composes them, the cell value, the index, the
value, evaluate, the update and the TD(0) step are the formulas of the definition on Python integers.  Boards are 16
exponents (0 = empty), row-major.

``value`` can leave a trace -- the (tuple, index) entry every look-up read -- so that a test can show from the reference
alone that its input reaches the edge it names.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

ILLEGAL = -(1 << 63)
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


@lru_cache(maxsize=None)
def shift_row(row):
    """game2048_env.py:243-260 on exponents: (new row, merge score).  Slide towards index 0, merge equal neighbours once,
    leftmost first.  A merge into exponent e scores 2^(e mod 32) -- the game's 2^e for every exponent play can reach."""
    tiles = [e for e in row if e != 0]
    out, score, k = [], 0, 0
    while k < len(tiles):
        if k + 1 < len(tiles) and tiles[k] == tiles[k + 1]:
            out.append(tiles[k] + 1)
            score += 1 << ((tiles[k] + 1) % 32)
            k += 2
        else:
            out.append(tiles[k])
            k += 1
    return tuple(out + [0] * (4 - len(out))), score


# cells of the four lines of a move in slide order (first cell = where tiles pile up): 0 up, 1 right, 2 down, 3 left
LINES = {
    0: [[c, c + 4, c + 8, c + 12] for c in range(4)],
    1: [[4 * r + 3, 4 * r + 2, 4 * r + 1, 4 * r] for r in range(4)],
    2: [[c + 12, c + 8, c + 4, c] for c in range(4)],
    3: [[4 * r, 4 * r + 1, 4 * r + 2, 4 * r + 3] for r in range(4)],
}


def move(b, d):
    """(afterstate, merge score, legal) of direction d on the 16-tuple b."""
    out, score = list(b), 0
    for line in LINES[d]:
        new, s = shift_row(tuple(b[c] for c in line))
        score += s
        for c, e in zip(line, new):
            out[c] = e
    out = tuple(out)
    return out, score % (1 << 31), out != b


def symmetries(b):
    """The eight boards training_data.augment() makes of b (training_data.py:257-299): the board and its horizontal
    flip, each turned clockwise by 0, 1, 2 and 3 quarter turns."""
    return [tuple(b[c] for c in perm) for perm in _sym_perms()]


@lru_cache(maxsize=None)
def _sym_perms():
    """numpy's flips and turns applied once, to the board of cell numbers: perm[c] = the cell that lands on c."""
    x = np.arange(16).reshape(4, 4)
    out = []
    for k in range(4):
        for base in (x, np.flip(x, 1)):
            out.append(tuple(int(e) for e in np.rot90(base, k, axes=(1, 0)).reshape(16)))
    return tuple(out)


def cell(e):
    return min(e % 32, 15)


def index(b, cells):
    return sum(cell(b[c]) << (4 * k) for k, c in enumerate(cells))


class Net:
    """tuples: T lists of L cell indices; weights: int64 array [T, 16^L] holding int32 values."""

    def __init__(self, tuples, frac_bits=10, weights=None):
        self.tuples = [tuple(t) for t in tuples]
        self.frac_bits = frac_bits
        shape = (len(self.tuples), 16 ** len(self.tuples[0]))
        self.weights = np.zeros(shape, np.int64) if weights is None else np.array(weights, np.int64).reshape(shape)

    def copy(self):
        return Net(self.tuples, self.frac_bits, self.weights.copy())


def plain(board):
    return tuple(int(x) % 32 for x in np.asarray(board).reshape(16))


def value(b, net, trace=None):
    """V(b); ``trace``: a list that receives the (t, idx) of each of the 8T look-ups."""
    v = 0
    for s in symmetries(b):
        for t, cells in enumerate(net.tuples):
            i = index(s, cells)
            v += int(net.weights[t, i])
            if trace is not None:
                trace.append((t, i))
    return v


def evaluate(board, net):
    """(q[4], action, best, after, after_value) of one board."""
    b = plain(board)
    q, after, vals = [ILLEGAL] * 4, [b] * 4, [0] * 4
    for d in range(4):
        a, g, legal = move(b, d)
        if legal:
            vals[d] = value(a, net)
            q[d] = (g << net.frac_bits) + vals[d]
            after[d] = a
    legal = [d for d in range(4) if q[d] != ILLEGAL]
    if not legal:
        return q, 0, 0, b, 0
    action = max(legal, key=lambda d: (q[d], -d))
    return q, action, q[action], after[action], vals[action]


def evaluate_batch(boards, net):
    """(value int64 [n, 4], action uint8 [n], best int64 [n], after uint8 [n, 16], after_value int64 [n])."""
    boards = np.asarray(boards).reshape(-1, 16)
    n = len(boards)
    val, act = np.zeros((n, 4), np.int64), np.zeros(n, np.uint8)
    best, after, av = np.zeros(n, np.int64), np.zeros((n, 16), np.uint8), np.zeros(n, np.int64)
    for i, b in enumerate(boards):
        q, act[i], best[i], a, av[i] = evaluate(b, net)
        val[i] = q
        after[i] = a
    return val, act, best, after, av


def values_batch(boards, net):
    return np.array([value(plain(b), net) for b in np.asarray(boards).reshape(-1, 16)], np.int64)


def step_of(delta, lr_shift):
    """sat_int32(delta >> lr_shift); Python's >> on ints is the arithmetic shift (it floors)."""
    return max(INT32_MIN, min(INT32_MAX, int(delta) >> lr_shift))


def wrap32(x):
    return (x + (1 << 31)) % (1 << 32) - (1 << 31)


def update(net, boards, deltas, lr_shift, trace=None):
    """In place.  ``trace``: a dict that counts "zero" steps, "sat" (saturated) steps and "wrap" (weights that wrapped)."""
    for b, delta in zip(np.asarray(boards).reshape(-1, 16), deltas):
        step = step_of(delta, lr_shift)
        if trace is not None:
            trace["zero"] = trace.get("zero", 0) + (step == 0)
            trace["sat"] = trace.get("sat", 0) + (step != int(delta) >> lr_shift)
        if step == 0:
            continue
        for s in symmetries(plain(b)):
            for t, cells in enumerate(net.tuples):
                i = index(s, cells)
                new = int(net.weights[t, i]) + step
                if trace is not None and wrap32(new) != new:
                    trace["wrap"] = trace.get("wrap", 0) + 1
                net.weights[t, i] = wrap32(new)


# ------------------------------------------------------------------------------------------------ the TD(0) trainer
def env_board(env):
    """Exponents of an oracle.cpu_ref.RefEnv (which holds tile values)."""
    return tuple(int(v).bit_length() - 1 if v else 0 for v in env.M)


def td_step(envs, net, lr_shift, trace=None):
    """One TD(0) step of every RefEnv under ``net`` (definition: evaluate, step with auto-reset, evaluate, update).
    ``trace``: a dict whose "episodes" counts the episodes that ended."""
    first = [evaluate(env_board(e), net) for e in envs]
    terminated = []
    for e, (_, action, *_rest) in zip(envs, first):
        _, term, _, _ = e.step(action)
        if term:
            e.reset()   # auto-reset: the next slots of the same transaction
        terminated.append(term)
    second = [evaluate(env_board(e), net) for e in envs]
    deltas = [(0 if term else s[2]) - f[4] for f, s, term in zip(first, second, terminated)]
    update(net, [f[3] for f in first], deltas, lr_shift)
    if trace is not None:
        trace["episodes"] = trace.get("episodes", 0) + sum(terminated)


def make_envs(n, seed, board_offset=0):
    from oracle.cpu_ref import RefEnv
    envs = [RefEnv(seed, board_offset + i) for i in range(n)]
    for e in envs:
        e.reset(seed)
    return envs


def greedy_actions(boards, net):
    return evaluate_batch(boards, net)[1]
