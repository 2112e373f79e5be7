"""Pure-Python reference of the n-tuple move log and backward learning (g2048_ntuple_play_log, g2048_ntuple_log_delta,
g2048_ntuple_log_sweep, g2048_ntuple_log_train), written from the definition in include/g2048.h: the rounds
of evaluate -> step(action, auto-reset) on the oracle that ntuple_td_helpers.reference_steps makes, kept in a log, and the
existing update references (ntuple_ref.update, ntuple_tc_ref.tc_update, ntuple_mean_ref.mean_update and their staged forms)
applied from the last slot to the first.  A plain module; nothing here calls the code under test."""
import types

import numpy as np

import late_game as lg
import ntuple_mean_ref as meanref
import ntuple_play_ref as pref
import ntuple_ref as ref
import ntuple_staged_ref as sref
import ntuple_tc_ref as tcref
from ntuple_play_helpers import ENGINEERED_CLOCK, cached
from ntuple_td_helpers import reference_steps, start_of

VALID, ENDED = 1, 2         # G2048_NTUPLE_LOG_VALID, G2048_NTUPLE_LOG_ENDED
M64 = (1 << 64) - 1


def wrap_i64(x):
    return ((int(x) + (1 << 63)) & M64) - (1 << 63)


def _mod(net):
    return ref if isinstance(net, ref.Net) else sref


class Log:
    """A zeroed log of depth M for n boards: after uint8 [M+1, n, 16], gain int64 [M+1, n], flag uint8 [M+1, n]."""

    def __init__(self, n, depth):
        self.n, self.depth = n, depth
        self.after = np.zeros((depth + 1, n, 16), np.uint8)
        self.gain = np.zeros((depth + 1, n), np.int64)
        self.flag = np.zeros((depth + 1, n), np.uint8)

    def copy(self):
        out = Log(self.n, self.depth)
        out.after, out.gain, out.flag = self.after.copy(), self.gain.copy(), self.flag.copy()
        return out


def assert_logs_equal(got, want, where):
    """``got`` and ``want``: anything with after / gain / flag arrays."""
    for name in ("flag", "gain", "after"):
        a, b = np.asarray(getattr(got, name)), np.asarray(getattr(want, name))
        assert a.shape == b.shape, f"{where}: {name} shape {a.shape} vs {b.shape}"
        assert np.array_equal(a, b), f"{where}: {name} differs at (slot, board) {np.argwhere(a != b)[:4, :2].tolist()}"


# ------------------------------------------------------------------------------------------------ play_log
def carry(log):
    """Point 1 of play_log: slot 0 takes the three entries slot M held."""
    log.after[0], log.gain[0], log.flag[0] = log.after[log.depth], log.gain[log.depth], log.flag[log.depth]


def write_move(log, m, best, after, after_value, no_move, terminated):
    """Point 2 of play_log for move m: the outputs of evaluate on the boards before the step, and the step's terminated."""
    log.after[m] = after
    log.gain[m] = np.array([wrap_i64(int(b) - int(v)) for b, v in zip(best, after_value)], np.int64)
    log.flag[m] = np.where(no_move, 0, VALID | np.where(np.asarray(terminated) != 0, ENDED, 0)).astype(np.uint8)


def oracle_of(n, max_exp=0):
    """The oracle reference_steps starts from: start_of(n) at late_game.BASE_OFFSET and ENGINEERED_CLOCK."""
    boards, scores = start_of(n)
    return pref.start_of(n, lg.SEED, lg.BASE_OFFSET, max_exp, boards=boards, scores=scores, clock=ENGINEERED_CLOCK)


def play_log(o, net, log):
    """play_log on the oracle ``o`` (advanced) under ``net`` (read): the carry, then M rounds of evaluate -> step.  Returns how
    many episodes ended per move."""
    carry(log)
    ended = []
    for m in range(1, log.depth + 1):
        _, action, best, after, after_value = _mod(net).evaluate_batch(o.boards, net)
        no_move = ~lg.legal_moves(o.boards).any(axis=1)
        o.step(action)
        write_move(log, m, best, after, after_value, no_move, o.terminated)
        ended.append(int((o.terminated != 0).sum()))
    return ended


def frozen_rounds(case, n, M, rounds, max_exp=0):
    """(reference_steps' result for M * rounds moves, [the log after each of ``rounds`` play_log calls]) under the case's
    weights, which nothing changes: the log filled from reference_steps' own per-step outputs.  Computed once."""
    def make():
        want = reference_steps(case, n, M * rounds, max_exp)
        best = _mod(case.rnet).evaluate_batch(want.start & 0x1f, case.rnet)[2]
        log, logs = Log(n, M), []
        for r in range(rounds):
            carry(log)
            for m in range(1, M + 1):
                j = r * M + m - 1
                s = want.steps[j]
                write_move(log, m, best, s.after, s.after_value, want.no_move[j], s.terminated)
                best = s.best_next
            logs.append(log.copy())
        return want, logs
    return cached(("log frozen", case.name, n, M, rounds, max_exp), make)


def reaches(logs):
    """From reference logs alone (the first round's and, when given, the second's): what the tests name before they compare."""
    first = logs[0]
    M = first.depth
    flags = np.concatenate([lg_.flag[1:].reshape(-1) for lg_ in logs])
    out = types.SimpleNamespace(values={int(f) for f in np.unique(flags)},
                                ended_below_M=bool(((first.flag[1:M] & ENDED) != 0).any()) if M > 1 else False,
                                ended_with_valid_successor=bool((((first.flag[:M] & ENDED) != 0) & ((first.flag[1:] & VALID) != 0)).any()),
                                empty_slot0=bool((first.flag[0] == 0).all()),
                                carried_slot0=len(logs) > 1 and bool(logs[1].after[0].any())
                                and np.array_equal(logs[1].flag[0], first.flag[M]) and np.array_equal(logs[1].after[0], first.after[M])
                                and np.array_equal(logs[1].gain[0], first.gain[M]),
                                carried_live=len(logs) > 1 and bool((logs[1].flag[0] != 0).any()),
                                live=int((flags != 0).sum()))
    return out


# ------------------------------------------------------------------------------------------------ log_delta
def log_delta(net, log, m, flag=None):
    """delta int64 [n] of slot m < M; ``flag``: another flag array to read (any bytes)."""
    assert 0 <= m < log.depth
    flag = log.flag if flag is None else flag
    values = _mod(net).values_batch
    out = np.zeros(log.n, np.int64)
    for i in range(log.n):
        f, f1 = int(flag[m, i]), int(flag[m + 1, i])
        if not f & VALID:
            continue
        v0 = int(values(log.after[m, i:i + 1], net)[0])
        if f & ENDED:
            out[i] = wrap_i64(0 - v0)
        elif f1 & VALID:
            out[i] = wrap_i64(int(log.gain[m + 1, i]) + int(values(log.after[m + 1, i:i + 1], net)[0]) - v0)
    return out


# ------------------------------------------------------------------------------------------------ sweep and train
def update_slot(net, log, m, delta, lr_shift, tc=None, mean=None):
    """The update of slot m by delta: TD, TC (phases 3) or batch-mean, by the existing references; in place."""
    boards = log.after[m]
    if tc is not None:
        (tcref if isinstance(net, ref.Net) else sref).tc_update(net, tc, boards, delta, lr_shift)
    elif mean is not None:
        meanref.mean_update(net, mean, boards, delta, lr_shift)
    else:
        _mod(net).update(net, boards, delta, lr_shift)


def sweep(net, log, lr_shift, tc=None, mean=None, order=None):
    """For m = M-1 down to 0 (``order``: another order of the slots, to show that it matters): log_delta(m), then the update of
    slot m.  In place on net (and tc / mean); returns the delta of the last slot visited."""
    delta = np.zeros(log.n, np.int64)
    for m in (range(log.depth - 1, -1, -1) if order is None else order):
        delta = log_delta(net, log, m)
        update_slot(net, log, m, delta, lr_shift, tc, mean)
    return delta


def train(o, net, log, rounds, lr_shift, tc=None, mean=None):
    """rounds x { play_log; sweep } on the oracle ``o``; in place on everything.  Returns the last sweep's last delta."""
    delta = np.zeros(log.n, np.int64)
    for _ in range(rounds):
        play_log(o, net, log)
        delta = sweep(net, log, lr_shift, tc, mean)
    return delta
