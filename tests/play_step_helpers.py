"""Shared by the budgeted play step tests (g2048_play_step): the reference of a step that takes its
actions from a table.  The unlimited trace is ``OracleBatch.step(actions[j])`` for j < k, in the shape of
``ntuple_play_ref.unlimited``; ``ntuple_play_ref.limited`` derives the budgeted form from it, as it does for the greedy
player.  The traces are computed once and never modified.  A plain module, like ntuple_play_helpers."""
import types

import numpy as np

import late_game as lg
import ntuple_play_ref as pref
from ntuple_play_helpers import ENGINEERED_CLOCK, budgets, cached, engineered

SEED = 77
K_TABLE = 64          # steps of the random table: an illegal move ends an episode, so random play finishes a game every few steps


def random_table(k, n, seed):
    """uint8 [k, n] of uniformly random actions 0..3."""
    return np.random.default_rng(seed).integers(0, 4, size=(k, n)).astype(np.uint8)


def unlimited(o, actions):
    """The trace of ``o.step(actions[j])`` for every row j of ``actions`` on the oracle ``o`` (which is advanced): the fields of
    ntuple_play_ref.unlimited."""
    k, n = actions.shape
    assert n == o.n
    tr = types.SimpleNamespace(n=n, k=k, t0=o.t, start=pref.records_of(o.boards, o.score), action=actions.astype(np.uint8),
                               terminated=np.zeros((k, n), bool), illegal=np.zeros((k, n), bool), gain=np.zeros((k, n), np.int64),
                               after=np.zeros((k, n, 16), np.uint8), terminal=np.zeros((k, n, 16), np.uint8),
                               terminal_score=np.zeros((k, n), np.int64))
    for j in range(k):
        o.step(actions[j])
        tr.terminated[j], tr.illegal[j] = o.terminated != 0, o.illegal != 0
        tr.gain[j] = np.where(tr.illegal[j], 0, o.reward).astype(np.int64)
        tr.after[j] = pref.records_of(o.boards, o.score)
        done = tr.terminated[j]
        tr.terminal[j][done] = pref.records_of(o.terminal_boards[done], o.last_score[done])
        tr.terminal_score[j][done] = o.last_score[done]
    return tr


def table_trace(n, k=K_TABLE, seed=SEED, board_offset=0, max_exp=0, table_seed=5):
    """(actions [k, n], the unlimited trace of them on n boards after reset())."""
    def make():
        actions = random_table(k, n, table_seed)
        return actions, unlimited(pref.start_of(n, seed, board_offset, max_exp), actions)
    return cached(("table", n, k, seed, board_offset, max_exp, table_seed), make)


def engineered_table_trace(k=12, table_seed=3):
    """The same from ntuple_play_helpers.engineered()'s late-game boards, at ENGINEERED_CLOCK and late_game.BASE_OFFSET, with the
    checks that they reach what they are there for: a dead board ends its episode on an illegal move whatever the action,
    a board with one hole ends or does not behind its spawn, and the score deficit carries (``table_seed`` is one of
    those whose table gets there)."""
    def make():
        boards, scores, dead, carry = engineered()
        actions = random_table(k, 96, table_seed)
        o = pref.start_of(96, lg.SEED, lg.BASE_OFFSET, boards=boards, scores=scores, clock=ENGINEERED_CLOCK)
        tr = unlimited(o, actions)
        assert tr.illegal[0, dead].all() and tr.terminated[0, dead].all()
        assert np.array_equal(tr.terminal[0, dead] & 0x1f, boards[dead])
        legal_hole = ~tr.illegal[0, :32]
        assert tr.terminated[0, :32][legal_hole].any() and not tr.terminated[0, :32][legal_hole].all()
        d = np.stack([lg.record_deficit(tr.start[carry])] + [lg.record_deficit(tr.after[j][carry]) for j in range(k)])
        # (as ntuple_play_helpers.engineered_trace: the first 4 spawned on a deficit of 2^k - 4 carries, across bit 12, around to 0)
        first = (d[:-1] == d[0]) & ((d[1:] - d[:-1]) % (1 << 24) == 4) & ~tr.terminated[:, carry]
        assert (first & (d[:-1] >= 4092)).any() and (first & ((d[:-1] ^ d[1:]) >> 12 != 0)).any() and (first & (d[1:] == 0)).any()
        return actions, tr
    return cached(("engineered-table", k, table_seed), make)


def assert_reaches(tr, want, budgeted=True):
    """What a table run is there for, from the reference's own trace."""
    hit = pref.reaches(tr, want)
    assert hit.two_episodes and hit.illegal_end and hit.directions == {0, 1, 2, 3}
    if budgeted:
        assert hit.ran_out and hit.never_moved


__all__ = ["SEED", "K_TABLE", "budgets", "random_table", "unlimited", "table_trace", "engineered_table_trace", "assert_reaches"]
