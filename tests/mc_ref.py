"""Pure-Python reference of the Monte-Carlo rollout search (include/g2048.h) -- TEST INFRASTRUCTURE ONLY.

Written from the definition with nothing from the device header: Philox is ``oracle.cpu_ref.philox4x32_10`` on Python
ints, a move slides four rows through ``shift_row`` (the game's rule written out cell by cell; tests/test_mc_host.py pins
it to the row table of tests/move_lut.py), the spawn is the ``floor(u * n)`` rule in Python integers.  Boards are 16
exponents (0 = empty), row-major, taken mod 32 as the plain entry point reads them.

Every playout can leave a trace -- how it ended and which candidate (1st..4th) each move needed -- so that a test can
show from the reference alone that its inputs reach the edges it claims.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

from oracle.cpu_ref import TWO_THRESHOLD, philox4x32_10

KEY_TAG = 0x4D435332
MASK32 = 0xFFFFFFFF


@lru_cache(maxsize=None)
def shift_row(row):
    """game2048_env.py:243-260 on exponents: (new row, merge score).  Slide towards index 0, merge equal neighbours once,
    leftmost first.  A merge into exponent e scores 2^(e mod 32); the row's score is kept mod 2^31, as the engine's
    32-bit per-move score is (exact below exponent 27, g2048_device.h)."""
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


def spawn(b, w):
    """add_tile from the 32-bit word w: position floor(u n) among the n empty cells in row-major order, u = w / 2^32;
    a 2 (exponent 1) when frac(u n) < 0.9, i.e. (w n mod 2^32) <= TWO_THRESHOLD, else a 4."""
    empty = [c for c in range(16) if b[c] == 0]
    p = w * len(empty)
    out = list(b)
    out[empty[p >> 32]] = 1 if (p & MASK32) <= TWO_THRESHOLD else 2
    return tuple(out)


def block(seed, i, d, r, j):
    return philox4x32_10((j & MASK32, r, i & MASK32, d), (seed & MASK32, ((seed >> 32) & MASK32) ^ KEY_TAG))


def playout(b, i, d, r, seed, L, trace=None):
    """(total score, moves after the root move) of playout r of root direction d, or None when d is illegal.
    ``trace``: a dict that receives ``end`` ("cap" / "terminal") and ``candidates`` (a 4-list: moves that took the
    1st..4th candidate)."""
    a, g, legal = move(b, d)
    if not legal:
        return None
    total, moves, cands, end = g, 0, [0, 0, 0, 0], None
    j = 0
    while True:
        if moves == L:
            end = "cap"
            break
        w = block(seed, i, d, r, j)
        a = spawn(a, w[0])
        a0 = w[1] >> 30
        for t in range(4):
            nxt, s, ok = move(a, (a0 + t) % 4)
            if ok:
                break
        else:
            end = "terminal"
            break
        a, total, moves = nxt, total + s, moves + 1
        cands[t] += 1
        j += 1
    if trace is not None:
        trace["end"], trace["candidates"] = end, cands
    return total, moves


def _plain(board):
    return tuple(int(x) % 32 for x in np.asarray(board).reshape(16))


def search(board, i, R, L, seed, stats=None):
    """(action, value[4], steps[4]) of one board with global index i.  ``stats``: a dict whose counters "cap",
    "terminal" and "candidates" (4-list) are increased by every playout."""
    b = _plain(board)
    value, steps = [-1] * 4, [-1] * 4
    for d in range(4):
        if not move(b, d)[2]:
            continue
        value[d] = steps[d] = 0
        for r in range(R):
            tr = {}
            total, moves = playout(b, i, d, r, seed, L, tr)
            value[d] += total
            steps[d] += moves
            if stats is not None:
                stats[tr["end"]] = stats.get(tr["end"], 0) + 1
                c = stats.setdefault("candidates", [0, 0, 0, 0])
                for k in range(4):
                    c[k] += tr["candidates"][k]
    action = 0 if max(value) < 0 else value.index(max(value))
    return action, value, steps


def search_batch(boards, R, L, seed, index_offset=0, stats=None):
    """(action uint8 [n], value int64 [n, 4], steps int64 [n, 4]); row k has global index index_offset + k."""
    boards = np.asarray(boards).reshape(-1, 16)
    act = np.zeros(len(boards), np.uint8)
    val = np.zeros((len(boards), 4), np.int64)
    stp = np.zeros((len(boards), 4), np.int64)
    for k, b in enumerate(boards):
        act[k], val[k], stp[k] = search(b, index_offset + k, R, L, seed, stats)
    return act, val, stp
