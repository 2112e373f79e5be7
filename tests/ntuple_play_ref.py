"""Reference model of n-tuple play (include/g2048.h "N-tuple play") -- TEST INFRASTRUCTURE ONLY.

Composed of what the suite already trusts and nothing of the code under test: ``oracle.OracleBatch.step(actions)`` makes the
step and ``evaluate_batch`` of ntuple_ref / ntuple_staged_ref (mixed networks: an ntuple_mixed_ref.mixed_net, which is a
StagedNet) chooses the action.  ``unlimited`` records the trace of K such rounds.  ``limited`` derives the budgeted form
from that trace: the spawn stream is a function of (transaction, board), so boards are independent, and a board's limited
trajectory is the prefix of its unlimited one through the reset after its G-th episode end, and constant from there on.
``hist``, ``moves`` and the final ``games_left`` are counted from the trace.
"""
from __future__ import annotations

import types

import numpy as np

import ntuple_ref as ref
import ntuple_staged_ref as sref
from late_game import potential
from oracle import OracleBatch

NO_LIMIT = (1 << 32) - 1
REACH_TILES = (2048, 4096, 8192, 16384, 32768)


def actions_of(boards, net):
    """The greedy player's action of every board: evaluate_batch of the reference the network belongs to."""
    return (ref if isinstance(net, ref.Net) else sref).evaluate_batch(boards, net)[1]


def records_of(boards, scores):
    """Engine records uint8 [n, 16] of plain boards and their scores: the cell in bits 0..4 and bit k of the deficit
    d = (potential - score) mod 2^24 in bit 5 + k % 3 of byte 8 + k // 3 (include/g2048.h)."""
    rec = np.array(boards, np.uint8).reshape(-1, 16)
    d = (potential(rec) - np.asarray(scores).astype(np.int64)) % (1 << 24)
    for k in range(24):
        rec[:, 8 + k // 3] |= (((d >> k) & 1) << (5 + k % 3)).astype(np.uint8)
    return rec


class Rows:
    """``[t, i]`` -> row t of a flat array, from ``bases[t]`` on: the weights of a mixed network too wide to pad (the
    references index ``weights[t, i]`` and nothing else)."""

    def __init__(self, flat, bases):
        self.flat, self.bases = flat, bases

    def __getitem__(self, ti):
        return self.flat[self.bases[ti[0]] + ti[1]]


def start_of(n, seed, board_offset=0, max_exp=0, boards=None, scores=None, clock=None):
    """An oracle after reset() -- or holding ``boards`` / ``scores`` at ``clock``, as an engine after set_boards, set_scores
    and set_clock."""
    o = OracleBatch(n, seed, board_offset)
    o.max_exp = max_exp
    if boards is None:
        o.reset()
    else:
        o.boards[:] = np.asarray(boards, np.uint8).reshape(n, 16)
        o.set_scores(np.zeros(n, np.int32) if scores is None else scores)
        o.t, o.fresh = clock, False
    return o


def unlimited(o, k_steps, net):
    """The trace of k_steps rounds of evaluate -> step(action, auto_reset) on the oracle ``o`` (which is advanced): per step j
    and board i the action, terminated, illegal, the merge score, the record after the step and its reset, and -- where the
    episode ended -- the terminal record."""
    n = o.n
    tr = types.SimpleNamespace(n=n, k=k_steps, t0=o.t, start=records_of(o.boards, o.score),
                               action=np.zeros((k_steps, n), np.uint8), terminated=np.zeros((k_steps, n), bool),
                               illegal=np.zeros((k_steps, n), bool), gain=np.zeros((k_steps, n), np.int64),
                               after=np.zeros((k_steps, n, 16), np.uint8), terminal=np.zeros((k_steps, n, 16), np.uint8),
                               terminal_score=np.zeros((k_steps, n), np.int64), boards=np.zeros((k_steps, n, 16), np.uint8))
    for j in range(k_steps):
        tr.boards[j] = o.boards
        tr.action[j] = actions_of(o.boards, net)
        o.step(tr.action[j])
        tr.terminated[j], tr.illegal[j] = o.terminated != 0, o.illegal != 0
        tr.gain[j] = np.where(tr.illegal[j], 0, o.reward).astype(np.int64)
        tr.after[j] = records_of(o.boards, o.score)
        done = tr.terminated[j]
        tr.terminal[j][done] = records_of(o.terminal_boards[done], o.last_score[done])
        tr.terminal_score[j][done] = o.last_score[done]
    return tr


def limited(tr, games_left=None):
    """What g2048_ntuple_play leaves behind after tr.k steps from tr.start, from the unlimited trace: ``games_left`` None is no
    limit.  Fields: records, games_left, played [k, n] (the board made step j), terminated [k, n], action [k, n] (0xff where
    not played), hist [32], moves, episodes [n], return_sum, gain_sum, last_records [n, 16] (zero: no episode ended), clock."""
    n, k = tr.n, tr.k
    budget = np.full(n, NO_LIMIT, np.int64) if games_left is None else np.asarray(games_left).astype(np.int64)
    ends_before = np.cumsum(tr.terminated, axis=0) - tr.terminated          # episode ends of board i before step j
    played = ends_before < budget[None, :]
    term = tr.terminated & played
    out = types.SimpleNamespace(played=played, terminated=term, clock=tr.t0 + k, moves=int(played.sum()),
                                episodes=term.sum(axis=0), gain_sum=int(tr.gain[played].sum()),
                                return_sum=int(tr.terminal_score[term].sum()))
    out.action = np.where(played, tr.action, 0xff).astype(np.uint8)
    out.records, out.last_records = tr.start.copy(), np.zeros((n, 16), np.uint8)
    for i in range(n):
        steps = np.nonzero(played[:, i])[0]
        if len(steps):
            out.records[i] = tr.after[steps[-1], i]
        ends = np.nonzero(term[:, i])[0]
        if len(ends):
            out.last_records[i] = tr.terminal[ends[-1], i]
    out.games_left = None if games_left is None else (budget - out.episodes).astype(np.uint32)
    out.hist = np.bincount((tr.terminal[term] & 0x1f).max(axis=1), minlength=32).astype(np.uint64) if term.any() else np.zeros(32, np.uint64)
    return out


def reach_of(hist):
    """{tile: share of the games whose highest tile was at least that tile}, from the tail sums of hist."""
    total = int(np.sum(hist))
    return {tile: (int(np.sum(hist[tile.bit_length() - 1:])) / total if total else 0.0) for tile in REACH_TILES}


def reaches(tr, out):
    """What a run reaches, from the reference's own trace: the facts a test names before it compares anything."""
    return types.SimpleNamespace(one_episode=bool((out.episodes >= 1).any()), two_episodes=bool((out.episodes >= 2).any()),
                                 directions=set(np.unique(out.action[out.played]).tolist()),
                                 illegal_end=bool((tr.illegal & out.played).any()),
                                 ran_out=bool((~out.played).any() and (out.played.any(axis=0) & ~out.played.all(axis=0)).any()),
                                 never_moved=bool((~out.played.any(axis=0)).any()))


def first_games(n, seed, net, cap, board_offset=0):
    """Every board's first game after reset(), played to its end or to ``cap`` steps: (score, highest exponent of the terminal
    board, moves), each int64 [n] with -1 / -1 / cap for a game unfinished at the cap.  Only boards whose first game is still
    running are evaluated (the others get action 0: boards are independent, what they do afterwards is not looked at)."""
    o = start_of(n, seed, board_offset)
    score, top, moves = np.full(n, -1, np.int64), np.full(n, -1, np.int64), np.full(n, cap, np.int64)
    for j in range(cap):
        live = score < 0
        if not live.any():
            break
        actions = np.zeros(n, np.uint8)
        actions[live] = actions_of(o.boards[live], net)
        o.step(actions)
        done = live & (o.terminated != 0)
        score[done], top[done], moves[done] = o.last_score[done], o.terminal_boards[done].max(axis=1), j + 1
    return score, top, moves
