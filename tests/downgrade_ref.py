"""Reference model of tile-downgrading (include/g2048.h "Tile-downgrading") -- TEST INFRASTRUCTURE ONLY.

``downgrade_one`` is the rule as the header states it, on one board, in plain Python; ``downgrade`` is the same rule on an
array, and tests/test_downgrade_host.py holds the two against each other.  ``unlimited`` is ntuple_play_ref.unlimited with the
greedy action taken on the translated board: the oracle makes the step, ``evaluate_batch`` of the references chooses the
action, nothing of the code under test is involved.  Its trace feeds ``ntuple_play_ref.limited`` unchanged.
"""
from __future__ import annotations

import types

import numpy as np

import ntuple_play_ref as pref

MIN_FLOOR = 4      # G2048_DOWNGRADE_MIN_FLOOR
SKIPPED = 0xff     # G2048_DOWNGRADE_SKIPPED


def downgrade_one(board, min_exp, floor_exp):
    """(translated board, k) of 16 bytes: every byte is read mod 32."""
    e = [int(x) & 0x1f for x in board]
    present = {x for x in e if x >= 1}
    twice = {x for x in present if e.count(x) >= 2}
    if not present:
        return e, 0
    m = max(present)
    if m < min_exp:
        return e, 0
    for c in range(m - 1, floor_exp - 1, -1):          # the LARGEST c in floor_exp .. m - 1
        if c not in present and (c - 1) not in twice:
            return [x - 1 if x > c else x for x in e], c
    return e, 0


def downgrade(boards, min_exp, floor_exp):
    """(uint8 [n, 16], uint8 [n]): the rule on every row of ``boards`` (uint8 [n, 16], bytes read mod 32)."""
    e = (np.asarray(boards, np.uint8).reshape(-1, 16) & 0x1f).astype(np.int64)
    n = len(e)
    counts = np.zeros((n, 33), np.int64)
    np.add.at(counts, (np.repeat(np.arange(n), 16), e.reshape(-1)), 1)
    counts[:, 0] = 0                                   # an empty cell is no tile
    present, twice = counts >= 1, counts >= 2
    c = np.arange(32)
    m = np.where(present.any(axis=1), 32 - np.argmax(present[:, ::-1], axis=1), 0)     # (index 32 is never set)
    below_twice = np.concatenate([np.zeros((n, 1), bool), twice[:, :31]], axis=1)       # (c - 1) in D
    ok = (c[None, :] >= floor_exp) & (c[None, :] < m[:, None]) & ~present[:, :32] & ~below_twice & (m >= min_exp)[:, None]
    k = np.where(ok.any(axis=1), 31 - np.argmax(ok[:, ::-1], axis=1), 0)
    out = e - ((k[:, None] != 0) & (e > k[:, None]))
    return out.astype(np.uint8), k.astype(np.uint8)


def unlimited(o, k_steps, net, min_exp, floor_exp):
    """ntuple_play_ref.unlimited on the oracle ``o`` with every action chosen on the translated board; the trace also holds
    ``missing`` [k, n] (the rule's k of the board each step began on) and ``plain_action`` [k, n] (the greedy action of the board
    itself), for the tests that must show the rule was at work."""
    n = o.n
    tr = types.SimpleNamespace(n=n, k=k_steps, t0=o.t, start=pref.records_of(o.boards, o.score),
                               action=np.zeros((k_steps, n), np.uint8), terminated=np.zeros((k_steps, n), bool),
                               illegal=np.zeros((k_steps, n), bool), gain=np.zeros((k_steps, n), np.int64),
                               after=np.zeros((k_steps, n, 16), np.uint8), terminal=np.zeros((k_steps, n, 16), np.uint8),
                               terminal_score=np.zeros((k_steps, n), np.int64), boards=np.zeros((k_steps, n, 16), np.uint8),
                               missing=np.zeros((k_steps, n), np.uint8), plain_action=np.zeros((k_steps, n), np.uint8))
    for j in range(k_steps):
        tr.boards[j] = o.boards
        low, tr.missing[j] = downgrade(o.boards, min_exp, floor_exp)
        tr.plain_action[j] = pref.actions_of(o.boards, net)
        tr.action[j] = tr.plain_action[j]
        moved = tr.missing[j] != 0
        if moved.any():
            tr.action[j][moved] = pref.actions_of(low[moved], net)
        o.step(tr.action[j])
        tr.terminated[j], tr.illegal[j] = o.terminated != 0, o.illegal != 0
        tr.gain[j] = np.where(tr.illegal[j], 0, o.reward).astype(np.int64)
        tr.after[j] = pref.records_of(o.boards, o.score)
        done = tr.terminated[j]
        tr.terminal[j][done] = pref.records_of(o.terminal_boards[done], o.last_score[done])
        tr.terminal_score[j][done] = o.last_score[done]
    return tr
