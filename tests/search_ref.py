"""Pure-Python reference of the expectimax search (include/g2048.h) -- TEST INFRASTRUCTURE ONLY.

Written from the definition, line by line and cell by cell, with nothing from the device header: moves are
``oracle.cpu_ref.RefEnv.move`` on tile values, the heuristic loops over the 4 rows and 4 columns, the chance node
over the empty cells in row-major order.  Boards are 16 exponents (0 = empty), row-major, taken mod 32 as the plain
entry point reads them.  Memoised on (board, depth): transpositions make depth 3 affordable in Python.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

from oracle.cpu_ref import IllegalMoveError, RefEnv

DEFAULT_WEIGHTS = (4096, 256, 128, 16)  # base, w_empty, w_merge, w_mono
MAX_WEIGHTS = (1 << 24, 65535, 65535, 65535)  # the largest the API accepts


def lines(b):
    """The 4 rows (left to right) and the 4 columns (top to bottom) of a 16-tuple."""
    return [tuple(b[4 * r + k] for k in range(4)) for r in range(4)] + [tuple(b[4 * k + c] for k in range(4)) for c in range(4)]


def line_terms(L):
    empty = sum(1 for x in L if x == 0)
    merge = sum(1 for i in range(3) if L[i] == L[i + 1] != 0)
    inc = sum(L[i] + L[i + 1] for i in range(3) if L[i] <= L[i + 1])
    dec = sum(L[i] + L[i + 1] for i in range(3) if L[i] >= L[i + 1])
    return empty, merge, max(inc, dec)


def heuristic(b, w=DEFAULT_WEIGHTS):
    base, w_empty, w_merge, w_mono = w
    h = base
    for L in lines(b):
        e, m, mono = line_terms(L)
        h += w_empty * e + w_merge * m + w_mono * mono
    return h


def move(b, m):
    """(afterstate, legal): RefEnv.move on tile values 2^e (game2048_env.py:194-241)."""
    env = RefEnv()
    env.M = [0 if e == 0 else 1 << e for e in b]
    try:
        env.move(m)
    except IllegalMoveError:
        return b, False
    return tuple(0 if v == 0 else v.bit_length() - 1 for v in env.M), True


@lru_cache(maxsize=None)
def _move_cached(b, m):
    return move(b, m)


@lru_cache(maxsize=None)
def value(b, d, w):
    """V_d(b)."""
    if d == 0:
        return heuristic(b, w)
    best = 0
    for m in range(4):
        a, legal = _move_cached(b, m)
        if legal:
            best = max(best, chance(a, d, w))
    return best


@lru_cache(maxsize=None)
def chance_total(a, d, w):
    """The undivided sum of C_d(a): 9 V(a + 2) + V(a + 4) over the empty cells (a 2 is exponent 1, a 4 exponent 2)."""
    total = 0
    for c in range(16):
        if a[c] == 0:
            total += 9 * value(a[:c] + (1,) + a[c + 1:], d - 1, w) + value(a[:c] + (2,) + a[c + 1:], d - 1, w)
    return total


def chance(a, d, w):
    """C_d(a): floor of the 9:1 weighted mean over the empty cells."""
    return chance_total(a, d, w) // (10 * sum(1 for x in a if x == 0))


def _plain(board):
    return tuple(int(x) % 32 for x in np.asarray(board).reshape(16))


def search(board, depth, w=DEFAULT_WEIGHTS):
    """(action, values[4]) of one board: values[m] = C_depth(move(b, m)), -1 if illegal; action = smallest argmax,
    0 when nothing is legal."""
    b, w = _plain(board), tuple(int(x) for x in w)
    vals = []
    for m in range(4):
        a, legal = _move_cached(b, m)
        vals.append(chance(a, depth, w) if legal else -1)
    action = max(range(4), key=lambda m: (vals[m], -m))
    return action, vals


def root_totals(board, depth, w=DEFAULT_WEIGHTS):
    """The four undivided root chance sums of ``search``: chance_total(move(b, m)), None where m is illegal."""
    b, w = _plain(board), tuple(int(x) for x in w)
    out = []
    for m in range(4):
        a, legal = _move_cached(b, m)
        out.append(chance_total(a, depth, w) if legal else None)
    return out


@lru_cache(maxsize=None)
def _max_exp_value(b, d):
    top = max(b)
    if d > 0:
        for m in range(4):
            a, legal = _move_cached(b, m)
            if legal:
                top = max(top, _max_exp_chance(a, d))
    return top


@lru_cache(maxsize=None)
def _max_exp_chance(a, d):
    top = max(a)
    for c in range(16):
        if a[c] == 0:
            top = max(top, _max_exp_value(a[:c] + (1,) + a[c + 1:], d - 1), _max_exp_value(a[:c] + (2,) + a[c + 1:], d - 1))
    return top


def max_exponent(board, depth):
    """The largest exponent on any board the depth-``depth`` search of ``board`` visits (merges can push it past 31)."""
    b = _plain(board)
    top = max(b)
    for m in range(4):
        a, legal = _move_cached(b, m)
        if legal:
            top = max(top, _max_exp_chance(a, depth))
    return top


def search_batch(boards, depth, w=DEFAULT_WEIGHTS):
    """uint8 [n, 16] -> (action uint8 [n], value int32 [n, 4])."""
    boards = np.asarray(boards).reshape(-1, 16)
    act = np.zeros(len(boards), np.uint8)
    val = np.zeros((len(boards), 4), np.int32)
    for i, b in enumerate(boards):
        act[i], val[i] = search(b, depth, w)
    return act, val


def _b(rows):
    return np.array(rows, np.uint8).reshape(16)


# Hand-made cases: name -> (board, depth, weights, expected action or None); the comment says what each one pins
HAND_CASES = {
    # only "right" (1) moves anything: the right column is free, the rest is a full board with no pairs
    "one_legal_move": (_b([[1, 2, 3, 0], [2, 3, 4, 0], [3, 4, 5, 0], [4, 5, 6, 0]]), 2, DEFAULT_WEIGHTS, 1),
    # a full board without equal neighbours: action 0, every value -1
    "dead": (_b([[1, 2, 1, 2], [2, 1, 2, 1], [1, 2, 1, 2], [2, 1, 2, 1]]), 2, DEFAULT_WEIGHTS, 0),
    # left-right mirror symmetric board: right (1) and left (3) tie exactly, up/down are illegal -> 1
    "tie_right_left": (_b([[1, 2, 2, 1], [3, 4, 4, 3], [5, 6, 6, 5], [7, 8, 8, 7]]), 1, DEFAULT_WEIGHTS, 1),
    # full board whose one pair (row 0) merges: the only empty cell of the afterstate comes from the merge
    "empty_from_merge": (_b([[1, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11], [12, 13, 14, 15]]), 3, DEFAULT_WEIGHTS, None),
    # all weights 0: every value is 0, the first legal move wins
    "zero_weights": (_b([[0, 1, 0, 0], [0, 0, 2, 0], [0, 0, 0, 0], [3, 0, 0, 1]]), 2, (0, 0, 0, 0), 0),
    # largest base and weights on a board with exponents near the top of the range
    "max_weights": (_b([[31, 31, 30, 0], [17, 17, 0, 2], [29, 0, 31, 1], [0, 30, 30, 30]]), 2, (1 << 24, 65535, 65535, 65535), None),
}
