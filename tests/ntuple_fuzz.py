#!/usr/bin/env python
"""N-tuple call-mix fuzz (test infrastructure; lives under tests/ because it drives the oracle and the pure-Python references):
random MIXES of the n-tuple calls -- evaluate, the searches, play, the learners, the move log, carousel, restart, tile-downgrading,
state save / restore -- against one model made of the existing references, every output and every piece of live state compared
bit for bit after every call.  tests/fuzz_parity.py does this for the environment engine; this is the same for what shares state
between the n-tuple calls: the engine's records, clock, ``terminated`` and episode books, the weights, ``NTupleTC.err`` / ``mag``,
``NTupleMean.sum`` / ``count`` (all zero between calls), the ``NTupleTrace`` / ``NTupleDelay`` rings, the ``NTupleLog`` (slot M is
carried into slot 0), the ``Carousel`` pools and the ``Restart`` snapshots and counters.

A case draws a network (ntuple_log_helpers.family_case: uniform and staged T = 1..8, mixed T = 2..8), n in {1, 63, 64, 65, 197, 257},
seed, board_offset, max_tile, start boards (fresh ones mixed with the engineered late-game boards of tests/late_game.py, scores set
-- below 2^24, where the record keeps them exactly; see SAFE_SCORE)
and the optional state owners (TC, Mean, Trace or Delay, Log, Carousel, Restart); then 12..30 calls.  Every draw depends on the
case's generator -- numpy's ``default_rng([seed, case])`` -- and on the MODEL's state only, never on anything read back from the
device: the same (seed, case) is the same call trace with or without a GPU, and one case replays alone.

The model (``Model``) owns one instance of each reference -- ntuple_staged_ref.StagedNet (a uniform network is one stage, a mixed
one the padded array of ntuple_mixed_ref), StagedTC, ntuple_mean_ref.Mean, ntuple_trace_ref.Trace, ntuple_delay_ref.Delay,
ntuple_log_ref.Log, carousel_ref.Carousel, restart_ref.State, downgrade_ref -- and the oracle batch as the engine, and has one
method per operation; the references are used as they are.  The searches take the host builds of the device header
(tests/host_ntuple_adaptive, tests/host_ntuple_reduced), pinned to the pure-Python references on one or two boards per call.  The
other side of the comparison is ``Device`` (the library) -- or a second ``Model``: tests/test_ntuple_fuzz_cpu.py runs the model
against sabotaged copies of itself to show that the comparison has teeth.

    python tests/ntuple_fuzz.py [seconds=120] [seed=0]        (G2048_FUZZ_STREAMS=1: every case on its own non-default stream)
    python tests/ntuple_fuzz.py --cases K [seed=0]            (K cases instead of a time budget: the run reproduces)
    python tests/ntuple_fuzz.py --replay SEED CASE            (one case alone: the same calls, the same mismatch message)
    (--model-only: no device, the oracle drives the model alone -- the call trace and the counters)"""
import hashlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

import carousel_ref as cref
import downgrade_ref as dgref
import late_game as lg
import ntuple_delay_ref as dref
import ntuple_log_ref as lref
import ntuple_mean_ref as meanref
import ntuple_mixed_ref as mref
import ntuple_play_ref as pref
import ntuple_reduced_ref as redref
import ntuple_ref as ref
import ntuple_staged_ref as sref
import ntuple_tc_ref as tcref
import ntuple_trace_ref as tref
import restart_ref as rr

ILLEGAL = ref.ILLEGAL
SIZES, SIZE_P = (1, 63, 64, 65, 197, 257), (0.12, 0.2, 0.2, 0.2, 0.14, 0.14)   # a lane; around a wavefront; 3 waves + a tail; a block + 1
LR_SHIFTS = (0, 6, 14, 40)                                 # 40: |delta| <= 2^40 >> 40 is 0 or -1 -- the zero weight step
LAMBDAS = (0.0, 0.5, 1.0, 0.8)
FORWARD = ("td", "tc", "mean", "tdl", "tcl", "mean_tdl", "delayed_tdl", "delayed_tcl")
OPS = (("evaluate_engine", "evaluate_plain", "values", "stage", "search1", "search2", "deep_search", "adaptive_search", "reduced_search",
        "downgrade_plain", "downgraded_boards", "play", "play_downgraded", "play_step", "engine_step")
       + tuple(f"{a}_{m}" for a in FORWARD for m in ("step", "train"))
       + ("delay_flush", "play_log_sweep", "backward_train", "copy_state", "mask_reset", "set_boards", "set_scores", "owner_reset", "refusal"))
EVENTS = ("episode_ended", "restart_made", "restart_refused_min_span", "restart_refused_max_restarts", "carousel_ride",
          "weight_step_zero", "weight_step_nonzero", "tc_nonzero_accumulators", "delay_item_due", "delay_flush", "log_carried_live",
          "downgrade_k_nonzero", "budget_ran_out", "no_legal_move")
# (seed, cases, every case on its own stream) of the pinned runs: tests/test_gpu_ntuple_fuzz.py runs them against the device,
# tests/test_ntuple_fuzz_cpu.py shows from the model alone that together they draw every operation and reach every event
PINNED = ((33, 8, False), (38, 8, True), (11, 8, False), (14, 8, True))
# The record keeps a score exactly below 2^24 (late_game.SCORE_LIMIT; include/g2048.h): the fuzz stays inside.  Scores it hands
# out are below SAFE_SCORE, a board within SCORE_GUARD of the limit makes set_scores the next call, and a case in which a score
# reaches the limit all the same is not compared any further (``OutOfDomain``: counted, never seen so far).
SAFE_SCORE, SCORE_GUARD = lg.SCORE_LIMIT - (1 << 22), 1 << 21
ORACLE_ROWS = ("boards", "score", "ep_start", "terminal_boards", "last_score", "last_len", "ep_count")
counts = {}
_host = {}


def bump(name, by=1):
    counts[name] = counts.get(name, 0) + int(by)


class Mismatch(AssertionError):
    """The two sides of the comparison differ; the message names seed, case, call, operation, parameters, field and indices."""


class OutOfDomain(Exception):
    """A score of the model reached 2^24: the case has left what the record keeps exactly (nothing is wrong with either side)."""


def host(name):
    """The host build of the adaptive ("adaptive") or reduced ("reduced") search, built on first use."""
    if name not in _host:
        import ntuple_adaptive_helpers as ah
        import ntuple_reduced_helpers as rh
        _host[name] = (ah.host_root, ah.load_host_adaptive()) if name == "adaptive" else (rh.host_root, rh.load_host_reduced())
    return _host[name]


def late_pool():
    """(boards uint8 [m, 16], scores int32 [m]): the 96 engineered late-game boards of ntuple_play_helpers (one empty cell, full
    and terminal, carrying score deficits) and 64 boards of late_game.high_family (tiles 2^12..2^17 at every fill level)."""
    from ntuple_play_helpers import cached, engineered

    def make():
        boards, scores, _, _ = engineered()
        high = lg.high_family(lg.SEED, 64)
        return (np.concatenate([boards, high.boards]).astype(np.uint8), np.concatenate([scores, high.scores]).astype(np.int32))
    return cached("ntuple fuzz late pool", make)


def digest(x):
    """A short, stable text of a parameter for the call trace: arrays by shape, dtype and a hash of their bytes."""
    if isinstance(x, np.ndarray):
        return f"{x.dtype}{list(x.shape)}#{hashlib.sha1(np.ascontiguousarray(x).tobytes()).hexdigest()[:10]}"
    if isinstance(x, dict):
        return "{" + ", ".join(f"{k}={digest(v)}" for k, v in x.items()) + "}"
    if isinstance(x, (tuple, list)):
        return "(" + ", ".join(digest(v) for v in x) + ")"
    return repr(x)


# ================================================================================================ the configuration of a case
class Config:
    """Everything a case draws before its first call."""

    def __init__(self, rs):
        from ntuple_log_helpers import family_case
        self.family = str(rs.choice(["uniform", "staged", "mixed"]))
        self.T = int(rs.integers(2 if self.family == "mixed" else 1, 9))
        self.net_case = family_case(self.family, self.T)
        self.n = n = int(rs.choice(SIZES, p=SIZE_P))
        self.seed = int(rs.integers(0, 2**63))
        self.offset = int(rs.choice([0, 12345, (1 << 32) - n, int(rs.integers(0, (1 << 32) - n))]))   # as fuzz_parity.py draws it
        max_tile = rs.choice([0, 0, 32, 2048])
        self.max_tile = int(max_tile) or None
        self.late = rs.random(n) < float(rs.choice([0.0, 0.5, 0.9]))              # which boards start late in a game
        self.late_pick = rs.integers(0, len(late_pool()[0]), n)
        self.fresh_scores = rs.integers(0, 1 << 20, n).astype(np.int32)
        self.tc = bool(rs.random() < 0.6)
        self.mean = bool(rs.random() < 0.5)
        self.ring = str(rs.choice(["none", "trace", "delay"], p=[0.2, 0.4, 0.4]))
        self.ring_depth = int(rs.choice([1, 2, 3, 4, 8]))
        self.lam = float(rs.choice(LAMBDAS))
        self.log_depth = int(rs.integers(1, 6)) if rs.random() < 0.6 else 0
        staged = self.net_case.stages is not None
        self.carousel = (int(rs.integers(1, 9)), int(rs.integers(0, 2**63))) if staged and rs.random() < 0.6 else None   # capacity, seed
        # small strides and capacities, as restart_ref.CASES: runs from late-game boards are short
        self.restart = (rr.Rule(k=int(rs.integers(0, 3)), C=int(rs.choice([1, 2, 4])), min_span=int(rs.choice([2, 3, 8])),
                                max_restarts=int(rs.choice([1, 2, rr.U32]))) if rs.random() < 0.6 else None)

    def __repr__(self):
        return (f"net={self.net_case.name} n={self.n} seed={self.seed} offset={self.offset} max_tile={self.max_tile} "
                f"late={int(self.late.sum())} tc={self.tc} mean={self.mean} ring={self.ring}(H={self.ring_depth}, lam={self.lam}) "
                f"log={self.log_depth} carousel={self.carousel} restart={self.restart}")


# ================================================================================================ the model
class Model:
    """One instance of each reference and the oracle batch; one method per operation: ``op_<name>(**params)`` applies the call and
    returns its outputs as a dict of numpy arrays / ints, ``state()`` returns every piece of live state.  ``events`` counts what
    the run reached.  The small ``_hooks`` are what the CPU test overrides to sabotage a copy."""

    def __init__(self, cfg):
        self.cfg, self.n, self.events = cfg, cfg.n, {}
        rnet = cfg.net_case.rnet
        self.net = (sref.StagedNet(rnet.tuples, (), rnet.frac_bits, rnet.weights.copy()[None]) if isinstance(rnet, ref.Net)
                    else rnet.copy())
        self.uniform = isinstance(rnet, ref.Net)
        self.mixed = len(set(mref.lens(self.net.tuples))) > 1
        self.tc = sref.StagedTC(self.net) if cfg.tc else None
        self.mean = meanref.Mean(self.net) if cfg.mean else None
        lam_q16 = int(round(cfg.lam * 65536))
        self.trace = tref.Trace(cfg.n, cfg.ring_depth, lam_q16) if cfg.ring == "trace" else None
        self.delay = dref.Delay(cfg.n, cfg.ring_depth, lam_q16) if cfg.ring == "delay" else None
        self.log = lref.Log(cfg.n, cfg.log_depth) if cfg.log_depth else None
        self.car = cref.Carousel(self.net.thr, cfg.n, cfg.carousel[0], cfg.carousel[1]) if cfg.carousel else None
        self.rst = rr.State(cfg.n, cfg.restart) if cfg.restart else None
        self.o = o = pref.OracleBatch(cfg.n, cfg.seed, cfg.offset)
        o.max_exp = cfg.max_tile.bit_length() - 1 if cfg.max_tile else 0
        o.reset()
        pool_boards, pool_scores = late_pool()
        self.start_boards = np.where(cfg.late[:, None], pool_boards[cfg.late_pick], o.boards).astype(np.uint8)
        self.start_scores = np.where(cfg.late, pool_scores[cfg.late_pick] % SAFE_SCORE, cfg.fresh_scores).astype(np.int32)
        o.boards[:] = self.start_boards
        o.set_scores(self.start_scores)
        self.terminated = np.zeros(cfg.n, np.uint8)
        self.last_records = np.zeros((cfg.n, 16), np.uint8)
        self.episodes = self.illegal_ends = 0

    def event(self, name, by=1):
        if by:
            self.events[name] = self.events.get(name, 0) + int(by)

    # ---------------------------------------------------------------------------------------------- the network
    def host_net(self):
        """The network for the host builds and the unstaged references: a view of the same weights."""
        return self.net.sub(0) if self.uniform else self.net

    def evaluate(self, boards):
        return sref.evaluate_batch(boards, self.net)

    def weights_flat(self, w):
        """A [S, T, 16^Lmax] array of the model in the layout of the device tensor, flattened."""
        w = mref.compact(w, self.net.tuples) if self.mixed else w
        return np.ascontiguousarray(w).reshape(-1)

    # ---------------------------------------------------------------------------------------------- the engine
    def records(self):
        return pref.records_of(self.o.boards, self.o.score)

    def _write_records(self, rec, before):
        """Records that a carousel or a restart replaced, back into the oracle: cells and the score the record carries."""
        o = self.o
        rows = np.nonzero((rec != before).any(axis=1))[0]
        if len(rows):
            o.boards[rows] = rec[rows] & 0x1f
            o.score[rows] = ((lg.potential(o.boards[rows]) - lg.record_deficit(rec[rows])) % lg.SCORE_LIMIT).astype(np.int32)

    def _step(self, actions, played=None, writes_terminated=False):
        """One engine step with auto-reset; ``played`` bool [n]: the other boards rest (a budgeted play).  Returns the step's
        terminated as bool [n]."""
        o = self.o
        self.event("no_legal_move", (~lg.legal_moves(o.boards).any(axis=1) & (True if played is None else played)).sum())
        masked = played is not None and not played.all()
        if masked:
            keep = {f: getattr(o, f).copy() for f in ORACLE_ROWS}
            gain_total, finished = o.gain_total, o.finished_return_sum
        o.step(None if actions is None else np.asarray(actions).astype(np.uint8) & 3)
        term, illegal = o.terminated != 0, o.illegal != 0
        if masked:
            term, illegal = term & played, illegal & played
            o.gain_total = gain_total + int(o.reward[played & ~illegal].astype(np.int64).sum())
            o.finished_return_sum = finished + int(o.last_score[term].astype(np.int64).sum())
        self.last_records[term] = pref.records_of(o.terminal_boards[term], o.last_score[term])
        self.episodes += int(term.sum())
        self.illegal_ends += int((term & illegal).sum())
        self.event("episode_ended", term.sum())
        if masked:
            rest = ~played
            for f in ORACLE_ROWS:
                getattr(o, f)[rest] = keep[f][rest]
        if writes_terminated:
            self.terminated = term.astype(np.uint8)
        return term

    def _ride(self, ride, term):
        """The carousel or restart step behind an engine step."""
        if ride == "carousel":
            rec, trace = self.records(), {}
            before = rec.copy()
            cref.step(self.car, rec, term, index_offset=self.o.board_offset, trace=trace)
            self.event("carousel_ride", sum(trace["restarts"]))
            self._write_records(rec, before)
        elif ride == "restart":
            rec = self.records()
            before = rec.copy()
            self._restart_step(rec, term)
            self._write_records(rec, before)

    def _restart_step(self, rec, term):
        ev = self.rst.events
        had = (ev.restarts, ev.refused_span, ev.refused_max)
        self.rst.step(rec, term)
        self.event("restart_made", ev.restarts - had[0])
        self.event("restart_refused_min_span", ev.refused_span - had[1])
        self.event("restart_refused_max_restarts", ev.refused_max - had[2])

    # ---------------------------------------------------------------------------------------------- read-only calls
    @staticmethod
    def _kept(names, keep, values):
        return {name: v for name, k, v in zip(names, keep, values) if k}

    def op_evaluate_engine(self, keep):
        return self._kept(("value", "action", "best", "after", "after_value"), keep, self.evaluate(self.o.boards))

    def op_evaluate_plain(self, boards, keep):
        return self._kept(("value", "action", "best", "after", "after_value"), keep, self.evaluate(boards))

    def op_values(self, boards):
        return {"values": sref.values_batch(boards, self.net)}

    def op_stage(self, boards):
        return {"stage": sref.stage_batch(boards, self.net.thr)}

    def _searched(self, boards, depths, active, R=None, check=()):
        """(action, value) of ``boards`` at ``depths`` [n] by the host build, rows with ``active`` 0 as the library leaves them;
        rows ``check`` also by the pure-Python reference, which must agree."""
        n = len(boards)
        act, val = np.zeros(n, np.uint8), np.full((n, 4), ILLEGAL, np.int64)
        fn, lib = host("adaptive" if R is None else "reduced")
        rnet = self.host_net()
        for d in np.unique(depths[active != 0]):
            rows = np.nonzero((depths == d) & (active != 0))[0]
            a, v = fn(lib, boards[rows], int(d), rnet) if R is None else fn(lib, boards[rows], int(d), R, rnet)
            act[rows], val[rows] = a, v
        for i in check:
            d = int(depths[i])
            if R is not None and self.uniform:
                v, a = redref.search(boards[i], d, R, rnet)
            elif R is None and d >= 1:
                v, a = sref.search(boards[i], d, self.net, {"memo": {}})
            else:
                continue
            assert a == act[i] and list(v) == val[i].tolist(), f"host build and reference disagree at depth {d} on {boards[i].tolist()}"
        return act, val

    def _fewest_empty(self, active, k):
        """The k active boards with the fewest empty cells: the ones the pure-Python search affords."""
        rows = np.nonzero(active != 0)[0]
        return rows[np.argsort((self.o.boards[rows] == 0).sum(axis=1), kind="stable")][:k]

    def op_search1(self):
        n = self.n
        active = np.ones(n, np.uint32)
        act, val = self._searched(self.o.boards, np.ones(n, np.int64), active, check=self._fewest_empty(active, 2))
        return {"action": act, "value": val}

    def op_search2(self, active):
        check = [i for i in self._fewest_empty(active, 1) if (self.o.boards[i] == 0).sum() <= 2]     # (about 0.1 s; a mid-game board: 0.75 s)
        act, val = self._searched(self.o.boards, np.full(self.n, 2), active, check=check)
        return {"action": act, "value": val}

    def op_deep_search(self, depth, active):
        act, val = self._searched(self.o.boards, np.full(self.n, depth), active)
        return {"action": act, "value": val}

    def op_adaptive_search(self, schedule, active):
        depths = np.asarray(schedule)[(self.o.boards == 0).sum(axis=1)]
        act, val = self._searched(self.o.boards, depths, active)
        return {"action": act, "value": val, "depth": np.where(active != 0, depths, 0xff).astype(np.uint8)}

    def op_reduced_search(self, schedule, reduce4, active):
        depths = np.asarray(schedule)[(self.o.boards == 0).sum(axis=1)]
        check = [i for i in self._fewest_empty(active, 1) if depths[i] <= 2]
        act, val = self._searched(self.o.boards, depths, active, R=reduce4, check=check)
        return {"action": act, "value": val, "depth": np.where(active != 0, depths, 0xff).astype(np.uint8)}

    def _downgrade(self, boards, rule):
        low, k = dgref.downgrade(boards, *rule)
        self.event("downgrade_k_nonzero", (k != 0).sum())
        return low, k

    def op_downgrade_plain(self, boards, rule):
        low, k = self._downgrade(boards, rule)
        return {"boards": low, "missing": k}

    def op_downgraded_boards(self, rule, active):
        low, k = self._downgrade(self.o.boards, rule)
        rest = active == 0
        low[rest], k[rest] = 0, dgref.SKIPPED
        return {"boards": low, "missing": k}

    # ---------------------------------------------------------------------------------------------- play
    def _budgeted(self, k_steps, budgets, actions_of):
        """k_steps budgeted steps; ``actions_of()`` gives the actions of the live boards or None (the synthetic policy)."""
        left = None if budgets is None else budgets.astype(np.int64)
        hist, moves = np.zeros(32, np.uint64), 0
        for _ in range(k_steps):
            played = np.ones(self.n, bool) if left is None else left > 0
            term = self._step(actions_of(), played)
            moves += int(played.sum())
            if term.any():
                hist += np.bincount((self.last_records[term] & 0x1f).max(axis=1), minlength=32).astype(np.uint64)
            if left is not None:
                left[term] -= 1
                self.event("budget_ran_out", (term & (left == 0)).sum())
        self._play_clock(k_steps)
        out = {"hist": hist, "moves": moves}
        if left is not None:
            out["games_left"] = left.astype(np.uint32)
        return out

    def _play_clock(self, k_steps):
        """The clock after a K-move launch: the oracle has already counted K transactions."""

    def op_play(self, k_steps, budgets):
        return self._budgeted(k_steps, budgets, lambda: self.evaluate(self.o.boards)[1])

    def op_play_downgraded(self, k_steps, budgets, rule):
        def actions():
            low, k = self._downgrade(self.o.boards, rule)
            return self.evaluate(np.where((k != 0)[:, None], low, self.o.boards))[1]
        return self._budgeted(k_steps, budgets, actions)

    def op_play_step(self, actions, dtype, budgets):
        return self._budgeted(1, budgets, lambda: actions)

    def op_engine_step(self, actions, dtype):
        o = self.o
        self._step(actions, writes_terminated=True)
        return {"reward": o.reward.copy(), "terminated": o.terminated.copy(), "illegal": o.illegal.copy(), "highest": o.highest.copy()}

    # ---------------------------------------------------------------------------------------------- the forward learners
    def _front(self, ride):
        """Evaluate, play the greedy move, the carousel or restart step, evaluate: the front half of every forward learner."""
        _, action, _, after, after_value = self.evaluate(self.o.boards)
        term = self._step(action, writes_terminated=True)
        self._ride(ride, term)
        best_next = self.evaluate(self.o.boards)[2]
        return action, after, after_value, best_next, term

    def _count_steps(self, deltas, lr_shift):
        steps = np.array([ref.step_of(d, lr_shift) for d in deltas])
        self.event("weight_step_zero", (steps == 0).sum())
        self.event("weight_step_nonzero", (steps != 0).sum())

    def _tc_update(self, fn, *args):
        """A temporal-coherence update of the references: ``fn(net, tc, *args)``."""
        self.event("tc_nonzero_accumulators", bool(self.tc.mag.any()))
        fn(self.net, self.tc, *args)

    def _mean_update(self, fn, *args):
        """A batch-mean update of the references: ``fn(net, mean, *args)``."""
        fn(self.net, self.mean, *args)

    def _push(self, ring, after, after_value, best_next, term):
        return (dref if ring is self.delay else tref).push(ring, after, after_value, best_next, term)

    def _delay_update(self, algo, lr_shift, mode):
        boards, _ = dref.due_items(self.delay, mode)
        if mode == dref.STEP:
            self.event("delay_item_due", len(boards))
        else:
            self.event("delay_flush")
        if algo == "delayed_tcl":
            self._tc_update(lambda net, tc: dref.tc_delay_update(net, tc, self.delay, lr_shift, 3, mode))
        else:
            dref.delay_update(self.net, self.delay, lr_shift, mode)

    def _forward_step(self, algo, lr_shift, ride):
        action, after, after_value, best_next, term = self._front(ride)
        net = self.net
        if algo in ("td", "tc", "mean"):
            delta = np.array([lref.wrap_i64((0 if t else int(b)) - int(v)) for b, v, t in zip(best_next, after_value, term)], np.int64)
            self._count_steps(delta, lr_shift)
            if algo == "td":
                sref.update(net, after, delta, lr_shift)
            elif algo == "tc":
                self._tc_update(sref.tc_update, after, delta, lr_shift)
            else:
                self._mean_update(meanref.mean_update, after, delta, lr_shift)
        elif algo in ("tdl", "tcl", "mean_tdl"):
            delta = self._push(self.trace, after, after_value, best_next, term)
            if algo == "tdl":
                sref.trace_update(net, self.trace, delta, lr_shift)
            elif algo == "tcl":
                self._tc_update(sref.tc_trace_update, self.trace, delta, lr_shift)
            else:
                self._mean_update(meanref.mean_trace_update, self.trace, delta, lr_shift)
        else:
            delta = self._push(self.delay, after, after_value, best_next, term)
            self._delay_update(algo, lr_shift, dref.STEP)
        return {"action": action, "after": after, "after_value": after_value, "best_next": best_next, "delta": delta}

    def op_forward(self, algo, mode, steps, lr_shift, fused, ride):
        out = {}
        for _ in range(steps):
            out = self._forward_step(algo, lr_shift, ride)
        if mode == "train":
            out = {}
            if algo.startswith("delayed"):
                self._delay_flush(algo, lr_shift)
        return out

    def _delay_flush(self, algo, lr_shift):
        """The flush and the reset that end a delayed trainer."""
        self._delay_update(algo, lr_shift, dref.FLUSH)
        self.delay.len[:] = 0

    def op_delay_flush(self, algo, lr_shift):
        self._delay_flush(algo, lr_shift)
        return {}

    # ---------------------------------------------------------------------------------------------- the move log
    def _log_carry(self):
        self.event("log_carried_live", bool((self.log.flag[self.log.depth] != 0).any()))
        lref.carry(self.log)

    def _play_log(self, restart):
        """ntuple_log_ref.play_log on this model's engine step, the restart step behind every move."""
        log = self.log
        self._log_carry()
        for m in range(1, log.depth + 1):
            _, action, best, after, after_value = self.evaluate(self.o.boards)
            no_move = ~lg.legal_moves(self.o.boards).any(axis=1)
            term = self._step(action)
            lref.write_move(log, m, best, after, after_value, no_move, term)
            if restart:
                self._ride("restart", term)
        self._play_clock(log.depth)

    def _sweep(self, lr_shift, which):
        tc, mean = (self.tc if which == "tc" else None), (self.mean if which == "mean" else None)
        if which == "tc":
            self.event("tc_nonzero_accumulators", bool(self.tc.mag.any()))
        return lref.sweep(self.net, self.log, lr_shift, tc, mean)

    def op_play_log_sweep(self, lr_shift, which, restart):
        self._play_log(restart)
        return {"delta": self._sweep(lr_shift, which)}

    def op_backward_train(self, rounds, lr_shift, which, restart):
        for _ in range(rounds):
            self._play_log(restart)
            self._sweep(lr_shift, which)
        return {}

    # ---------------------------------------------------------------------------------------------- state
    def op_copy_state(self):
        self.terminated[:] = 0                     # ``terminated`` is an output buffer of the engine object, not engine state
        return {}

    def op_mask_reset(self, mask):
        self.o.reset(mask=mask)
        return {}

    def op_set_boards(self, boards, scores):
        self.o.boards[:] = boards
        self.o.set_scores(scores)
        return {}

    def op_set_scores(self, scores, on_device):
        self.o.set_scores(scores)
        return {}

    def in_domain(self):
        return max(int(self.o.score.max()), int(self.o.last_score.max())) < lg.SCORE_LIMIT

    def op_owner_reset(self, owner):
        if owner in ("trace", "delay"):
            getattr(self, owner).len[:] = 0
        elif owner == "restart":
            self.rst.pos[:], self.rst.start[:], self.rst.restarts[:] = 0, 0, 0
        elif owner == "log":
            self.log.after[:], self.log.gain[:], self.log.flag[:] = 0, 0, 0
        else:
            self.car.seen[:] = cref.UNKNOWN
        return {}

    def op_refusal(self, kind):
        return {}                                  # refused before anything is launched: nothing changes

    def state(self):
        """Every piece of live state, by name, in the order the comparison reports differences."""
        o = self.o
        s = {"records": self.records(), "clock": o.t, "terminated": self.terminated, "episodes": self.episodes,
             "illegal_ends": self.illegal_ends, "return_sum": o.return_sum, "last_records": self.last_records,
             "last_scores": o.last_score.copy()}
        for name, ring in (("trace", self.trace), ("delay", self.delay)):
            if ring is not None:
                s[name + ".hist"], s[name + ".len"], s[name + ".slot"] = ring.hist, ring.len, ring.slot
        if self.delay is not None:
            s["delay.acc"] = self.delay.acc_i64()
        if self.log is not None:
            s["log.after"], s["log.gain"], s["log.flag"] = self.log.after, self.log.gain, self.log.flag
        if self.car is not None:
            c = self.car
            s["carousel.pool"], s["carousel.count"], s["carousel.seen"] = c.pool, c.count_i64(), c.seen
            s["carousel.episodes"] = c.episodes.view(np.int32)
        if self.rst is not None:
            r = self.rst
            s["restart.snap"] = r.snap
            s["restart.pos"], s["restart.start"], s["restart.restarts"] = (x.view(np.int32) for x in (r.pos, r.start, r.restarts))
        # the tables last: a difference in a ring, a log or a rider is named before the weights it has moved since
        if self.mean is not None:
            s["mean.sum"], s["mean.count"] = self.weights_flat(self.mean.sum), self.weights_flat(self.mean.count).view(np.int32)
        if self.tc is not None:
            s["tc.err"], s["tc.mag"] = self.weights_flat(self.tc.err), self.weights_flat(self.tc.mag_i64())
        s["weights"] = self.weights_flat(self.net.weights).astype(np.int32)
        return s

    def close(self):
        pass


# ================================================================================================ the device
class Device:
    """The library under the same operations: every ``op_<name>`` takes the parameters the model's takes and returns the same
    outputs, read back as numpy; ``state()`` reads every piece of live state back."""

    def __init__(self, cfg, model):
        import torch
        import gym2048_amd as g
        from gym2048_amd import ntuple
        from ntuple_log_helpers import net_of
        self.torch, self.g, self.nt, self.cfg, self.n = torch, g, ntuple, cfg, cfg.n
        self.eng = g.Batched2048(cfg.n, seed=cfg.seed, board_offset=cfg.offset, max_tile=cfg.max_tile)
        self.dev = self.eng.device
        self.eng.reset()
        self.eng.set_boards(model.start_boards)
        self.eng.set_scores(model.start_scores)
        self.net = net_of(g, torch, cfg.net_case)
        n = cfg.n
        self.tc = g.NTupleTC(self.net) if cfg.tc else None
        self.mean = g.NTupleMean(self.net) if cfg.mean else None
        self.trace = g.NTupleTrace(n, depth=cfg.ring_depth, lam=cfg.lam) if cfg.ring == "trace" else None
        self.delay = g.NTupleDelay(n, depth=cfg.ring_depth, lam=cfg.lam) if cfg.ring == "delay" else None
        self.log = g.NTupleLog(n, depth=cfg.log_depth) if cfg.log_depth else None
        self.car = g.Carousel(self.net, n, capacity=cfg.carousel[0], seed=cfg.carousel[1]) if cfg.carousel else None
        self.rst = self._new_restart(n) if cfg.restart else None
        self.work = ntuple.td_work(self.eng)

    def _new_restart(self, n):
        r = self.cfg.restart
        return self.g.Restart(n, stride=1 << r.k, capacity=r.C, min_span=r.min_span, max_restarts=r.max_restarts)

    # ---------------------------------------------------------------------------------------------- conversions
    def to(self, a, dtype=None):
        t = self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        return t if dtype is None else t.to(dtype)

    def u32(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(self.dev).view(self.torch.uint32)

    def u64_zeros(self, k):
        return self.torch.zeros(k, dtype=self.torch.int64, device=self.dev).view(self.torch.uint64)

    @staticmethod
    def np_(t):
        """A device tensor as numpy; the unsigned 32- and 64-bit ones through their signed views."""
        import torch
        if t.dtype == torch.uint32:
            return t.view(torch.int32).cpu().numpy().view(np.uint32)
        if t.dtype == torch.uint64:
            return t.view(torch.int64).cpu().numpy().view(np.uint64)
        return t.cpu().numpy()

    def _out(self, names, keep, shapes_dtypes):
        t = self.torch
        return [t.empty(sh, dtype=dt, device=self.dev) if k else None for k, (sh, dt) in zip(keep, shapes_dtypes)]

    def _eval_out(self, n, keep):
        t = self.torch
        return self.nt.NTupleEval(*self._out(None, keep, (((n, 4), t.int64), ((n,), t.uint8), ((n,), t.int64), ((n, 16), t.uint8),
                                                           ((n,), t.int64))))

    def _named(self, result):
        return {name: self.np_(v) for name, v in result._asdict().items() if v is not None}

    # ---------------------------------------------------------------------------------------------- read-only calls
    def op_evaluate_engine(self, keep):
        return self._named(self.eng.ntuple_evaluate(self.net, out=self._eval_out(self.n, keep)))

    def op_evaluate_plain(self, boards, keep):
        return self._named(self.net.evaluate(self.to(boards), out=self._eval_out(len(boards), keep)))

    def op_values(self, boards):
        return {"values": self.np_(self.net.values(self.to(boards)))}

    def op_stage(self, boards):
        return {"stage": self.np_(self.net.stage(self.to(boards)))}

    def op_search1(self):
        return self._named(self.eng.ntuple_search(self.net, 1))

    def op_search2(self, active):
        return self._named(self.eng.ntuple_search(self.net, 2, active=self.u32(active)))

    def op_deep_search(self, depth, active):
        return self._named(self.eng.ntuple_deep_search(self.net, depth, active=self.u32(active)))

    def op_adaptive_search(self, schedule, active):
        return self._named(self.eng.ntuple_adaptive_search(self.net, schedule, active=self.u32(active)))

    def op_reduced_search(self, schedule, reduce4, active):
        return self._named(self.eng.ntuple_reduced_search(self.net, schedule, reduce4, active=self.u32(active)))

    def _rule(self, rule):
        return self.g.Downgrade(min_tile=1 << rule[0], floor_tile=1 << rule[1])

    def op_downgrade_plain(self, boards, rule):
        return self._named(self.nt.downgrade(self.to(boards), self._rule(rule)))

    def op_downgraded_boards(self, rule, active):
        return self._named(self.eng.downgraded_boards(self._rule(rule), active=self.u32(active)))

    # ---------------------------------------------------------------------------------------------- play
    def _side(self, budgets):
        left = None if budgets is None else self.u32(budgets)
        return left, self.u64_zeros(32), self.u64_zeros(1)

    def _side_out(self, left, hist, moves):
        out = {"hist": self.np_(hist), "moves": int(self.np_(moves)[0])}
        if left is not None:
            out["games_left"] = self.np_(left)
        return out

    def op_play(self, k_steps, budgets, rule=None):
        left, hist, moves = self._side(budgets)
        self.eng.ntuple_play(self.net, k_steps, games_left=left, hist=hist, moves=moves, downgrade=None if rule is None else self._rule(rule))
        return self._side_out(left, hist, moves)

    def op_play_downgraded(self, k_steps, budgets, rule):
        return self.op_play(k_steps, budgets, rule)

    def _actions(self, actions, dtype):
        return None if actions is None else self.to(actions, getattr(self.torch, dtype))

    def op_play_step(self, actions, dtype, budgets):
        left, hist, moves = self._side(budgets)
        self.eng.play_step(self._actions(actions, dtype), games_left=left, hist=hist, moves=moves)
        return self._side_out(left, hist, moves)

    def op_engine_step(self, actions, dtype):
        e = self.eng
        e.step(self._actions(actions, dtype), auto_reset=True)
        return {name: self.np_(getattr(e, name)) for name in ("reward", "terminated", "illegal", "highest")}

    # ---------------------------------------------------------------------------------------------- the learners
    def _riders(self, ride):
        return {"carousel": {"carousel": self.car}, "restart": {"restart": self.rst}}.get(ride, {})

    def _owners(self, algo):
        """The state owners a forward learner takes between ``net`` and ``lr_shift``, in its order."""
        return {"td": (), "tc": (self.tc,), "mean": (self.mean,), "tdl": (self.trace,), "tcl": (self.tc, self.trace),
                "mean_tdl": (self.mean, self.trace), "delayed_tdl": (self.delay,), "delayed_tcl": (self.tc, self.delay)}[algo]

    def op_forward(self, algo, mode, steps, lr_shift, fused, ride):
        nt, kw = self.nt, dict(fused=fused, **self._riders(ride))
        if mode == "train":
            getattr(nt, "train" if algo == "td" else algo + "_train")(self.eng, self.net, *self._owners(algo), steps, lr_shift, **kw)
            return {}
        w = getattr(nt, algo + "_step")(self.eng, self.net, *self._owners(algo), lr_shift, self.work, **kw)
        return {"action": self.np_(w.before.action), "after": self.np_(w.before.after), "after_value": self.np_(w.before.after_value),
                "best_next": self.np_(w.after.best), "delta": self.np_(w.delta)}

    def op_delay_flush(self, algo, lr_shift):
        if algo == "delayed_tcl":
            self.net.tc_delay_update(self.delay, lr_shift, self.tc, flush=True)
        else:
            self.net.delay_update(self.delay, lr_shift, flush=True)
        self.delay.reset()
        return {}

    def _which(self, which):
        return dict(tc=self.tc if which == "tc" else None, mean=self.mean if which == "mean" else None)

    def op_play_log_sweep(self, lr_shift, which, restart):
        self.eng.ntuple_play_log(self.net, self.log, restart=self.rst if restart else None)
        return {"delta": self.np_(self.nt.log_sweep(self.net, self.log, lr_shift, **self._which(which)))}

    def op_backward_train(self, rounds, lr_shift, which, restart):
        self.nt.backward_train(self.eng, self.net, self.log, rounds, lr_shift, restart=self.rst if restart else None, **self._which(which))
        return {}

    # ---------------------------------------------------------------------------------------------- state
    def op_copy_state(self):
        """``state_dict()`` of every owner into freshly constructed objects, the engine's state into a second engine; the run
        goes on with the copies."""
        g, cfg, n = self.g, self.cfg, self.n
        case = cfg.net_case
        net = g.NTupleNet(case.tuples, frac_bits=case.rnet.frac_bits, stages=case.stages, mixed=True)
        net.load_state_dict(self.net.state_dict())
        fresh = {"net": net}
        if self.tc is not None:
            fresh["tc"] = g.NTupleTC(net)
            fresh["tc"].load_state_dict(self.tc.state_dict())
        if self.mean is not None:
            fresh["mean"] = g.NTupleMean(net)                # (no state: all zero between calls)
        for name, cls in (("trace", g.NTupleTrace), ("delay", g.NTupleDelay)):
            if getattr(self, name) is not None:
                fresh[name] = cls(n, depth=cfg.ring_depth, lam=cfg.lam)
                fresh[name].load_state_dict(getattr(self, name).state_dict())
        if self.log is not None:
            fresh["log"] = g.NTupleLog(n, depth=cfg.log_depth)
            fresh["log"].load_state_dict(self.log.state_dict())
        if self.car is not None:
            fresh["car"] = g.Carousel(net, n, capacity=cfg.carousel[0], seed=cfg.carousel[1])
            fresh["car"].load_state_dict(self.car.state_dict())
        if self.rst is not None:
            fresh["rst"] = self._new_restart(n)
            fresh["rst"].load_state_dict(self.rst.state_dict())
        other = g.Batched2048(n, seed=1, board_offset=0)
        other.load_state_dict(self.eng.state_dict())
        other.set_max_tile(cfg.max_tile)
        self.eng.close()
        self.eng = other
        for name, obj in fresh.items():
            setattr(self, name, obj)
        self.work = self.nt.td_work(self.eng)
        return {}

    def op_mask_reset(self, mask):
        self.eng.reset(mask=mask)
        return {}

    def op_set_boards(self, boards, scores):
        self.eng.set_boards(boards)
        self.eng.set_scores(scores)
        return {}

    def op_set_scores(self, scores, on_device):
        self.eng.set_scores(self.to(scores) if on_device else scores)
        return {}

    def op_owner_reset(self, owner):
        {"trace": self.trace, "delay": self.delay, "restart": self.rst, "log": self.log, "carousel": self.car}[owner].reset()
        return {}

    def op_refusal(self, kind):
        """A combination the documentation refuses, each checked before anything is launched: ValueError, and (the state
        comparison that follows every call) nothing on the device changed."""
        nt, eng, net = self.nt, self.eng, self.net
        calls = {
            "carousel_and_restart": lambda: nt.td_step(eng, net, 6, self.work, carousel=self.car, restart=self.rst),
            "fused_with_restart": lambda: nt.tc_step(eng, net, self.tc, 6, self.work, fused=True, restart=self.rst),
            "fused_with_carousel": lambda: nt.train(eng, net, 2, 6, carousel=self.car, fused=True),
            "restart_of_another_size": lambda: nt.td_step(eng, net, 6, self.work, restart=self._new_restart(self.n + 1)),
            "backward_train_with_carousel": lambda: nt.backward_train(eng, net, self.log, 1, 6, carousel=self.car),
            "sweep_with_tc_and_mean": lambda: nt.log_sweep(net, self.log, 6, tc=self.tc, mean=self.mean),
        }
        try:
            calls[kind]()
        except ValueError:
            return {}
        raise AssertionError(f"{kind}: no ValueError")

    def state(self):
        e, np_ = self.eng, self.np_
        st = e.episode_stats()
        s = {"records": np_(e.records()), "clock": e.clock, "terminated": np_(e.terminated), "episodes": st["episodes"],
             "illegal_ends": st["illegal_ends"], "return_sum": st["return_sum"], "last_records": np_(e.last_records()),
             "last_scores": e.get_last_scores(), "weights": np_(self.net.weights).reshape(-1)}
        if self.tc is not None:
            s["tc.err"], s["tc.mag"] = np_(self.tc.err).reshape(-1), np_(self.tc.mag).reshape(-1)
        if self.mean is not None:
            s["mean.sum"], s["mean.count"] = np_(self.mean.sum).reshape(-1), np_(self.mean.count).reshape(-1)
        for name, ring in (("trace", self.trace), ("delay", self.delay)):
            if ring is not None:
                s[name + ".hist"], s[name + ".len"], s[name + ".slot"] = np_(ring.hist), np_(ring.len), ring.slot
        if self.delay is not None:
            s["delay.acc"] = np_(self.delay.acc)
        if self.log is not None:
            s["log.after"], s["log.gain"], s["log.flag"] = np_(self.log.after), np_(self.log.gain), np_(self.log.flag)
        if self.car is not None:
            c = self.car
            s["carousel.pool"], s["carousel.count"], s["carousel.seen"] = np_(c.pool), np_(c.count), np_(c.seen)
            s["carousel.episodes"] = np_(c.episodes)
        if self.rst is not None:
            r = self.rst
            s["restart.snap"], s["restart.pos"], s["restart.start"], s["restart.restarts"] = (np_(x) for x in (r.snap, r.pos, r.start, r.restarts))
        return s

    def close(self):
        self.eng.close()


# ================================================================================================ the calls of a case
def _subset(rs, n, k=4):
    """A uint32 [n] mask with at most k boards on."""
    active = np.zeros(n, np.uint32)
    active[rs.choice(n, size=min(n, int(rs.integers(1, k + 1))), replace=False)] = rs.integers(1, 4)
    return active


def _keep(rs, k):
    keep = [bool(rs.random() < 0.6) for _ in range(k)]
    keep[int(rs.integers(0, k))] = True
    return tuple(keep)


def _plain_boards(rs, model):
    """A batch of plain boards for the plain forms: the live boards, late-game boards and random cells mod 32, mixed."""
    m = int(rs.choice([1, 7, 64, 65, 130]))
    pool = late_pool()[0]
    live = model.o.boards[rs.integers(0, model.n, m)]
    late = pool[rs.integers(0, len(pool), m)]
    rand = ((rs.integers(0, 18, (m, 16)) * (rs.random((m, 16)) < 0.7)) | (rs.integers(0, 8, (m, 16)) << 5)).astype(np.uint8)
    pick = rs.integers(0, 3, m)[:, None]
    return np.where(pick == 0, live, np.where(pick == 1, late, rand)).astype(np.uint8)


def _budgets(rs, n):
    if rs.random() < 0.4:
        return None
    b = rs.choice(np.array([0, 1, 1, 2, pref.NO_LIMIT], np.uint32), n)
    return b.astype(np.uint32)


def _rule(rs):
    """(min_exp, floor_exp) of a tile-downgrading rule."""
    return (int(rs.choice([3, 6, 11, 15])), int(rs.choice([4, 5, 8])))


def _schedule(rs):
    """17 depths, deep only where a board has few empty cells (the cost of a ply grows steeply with them)."""
    cap = [4, 3, 3, 3, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]
    return tuple(int(rs.integers(0, c + 1)) for c in cap)


def _actions(rs, n):
    """(actions uint8 [n] in 0..3, the dtype the device tensor gets), or (None, ...): the synthetic policy."""
    if rs.random() < 0.25:
        return None, "uint8"
    dtype = str(rs.choice(["uint8", "int32", "int64"]))
    return rs.integers(0, 4, n).astype(np.uint8), dtype


def draw_call(rs, model):
    """(operation kind, model / device method, parameters) of the next call, from the generator and the model's state."""
    cfg, n = model.cfg, model.n
    if int(model.o.score.max()) >= lg.SCORE_LIMIT - SCORE_GUARD:
        return "set_scores", "set_scores", dict(scores=rs.integers(0, 1 << 20, n).astype(np.int32), on_device=bool(rs.random() < 0.5))
    staged = cfg.net_case.stages is not None
    rides = ["none"] + (["carousel"] if model.car is not None else []) + (["restart", "restart"] if model.rst is not None else [])
    algos = ["td"] + (["tc"] if model.tc else []) + (["mean"] if model.mean else [])
    if model.trace is not None:
        algos += ["tdl"] + (["tcl"] if model.tc else []) + (["mean_tdl"] if model.mean else [])
    if model.delay is not None:
        algos += ["delayed_tdl"] + (["delayed_tcl"] if model.tc else [])
    group = str(rs.choice(["read", "play", "learn", "log", "state"], p=[0.22, 0.16, 0.4, 0.12, 0.1]))
    if group == "log" and model.log is None:
        group = "learn"
    if group == "read":
        kind = str(rs.choice(["evaluate_engine", "evaluate_plain", "values", "stage", "search1", "search2", "deep_search", "adaptive_search",
                              "reduced_search", "downgrade_plain", "downgraded_boards"]))
        if kind == "stage" and not staged:
            kind = "values"
        if kind == "evaluate_engine":
            return kind, kind, dict(keep=_keep(rs, 5))
        if kind == "evaluate_plain":
            return kind, kind, dict(boards=_plain_boards(rs, model), keep=_keep(rs, 5))
        if kind in ("values", "stage"):
            return kind, kind, dict(boards=_plain_boards(rs, model))
        if kind == "search1":
            return kind, kind, {}
        if kind == "search2":
            return kind, kind, dict(active=_subset(rs, n))
        if kind == "deep_search":
            active = _subset(rs, n)
            few = int((model.o.boards[active != 0] == 0).sum(axis=1).max()) <= 4        # (from the model's boards)
            return kind, kind, dict(depth=3 if few and rs.random() < 0.7 else 2, active=active)
        if kind == "adaptive_search":
            return kind, kind, dict(schedule=_schedule(rs), active=_subset(rs, n))
        if kind == "reduced_search":
            return kind, kind, dict(schedule=_schedule(rs), reduce4=int(rs.integers(1, 3)), active=_subset(rs, n))
        if kind == "downgrade_plain":
            return kind, kind, dict(boards=_plain_boards(rs, model), rule=_rule(rs))
        return kind, kind, dict(rule=_rule(rs), active=(rs.random(n) < 0.7).astype(np.uint32) * 3)
    if group == "play":
        kind = str(rs.choice(["play", "play_downgraded", "play_step", "engine_step"]))
        if kind == "play":
            return kind, kind, dict(k_steps=int(rs.integers(1, 6)), budgets=_budgets(rs, n))
        if kind == "play_downgraded":
            return kind, kind, dict(k_steps=int(rs.integers(1, 6)), budgets=_budgets(rs, n), rule=_rule(rs))
        actions, dtype = _actions(rs, n)
        if kind == "play_step":
            return kind, kind, dict(actions=actions, dtype=dtype, budgets=_budgets(rs, n))
        return kind, kind, dict(actions=actions, dtype=dtype)
    if group == "learn":
        algo = str(rs.choice(algos))
        if algo.startswith("delayed") and rs.random() < 0.15:
            return "delay_flush", "delay_flush", dict(algo=algo, lr_shift=int(rs.choice(LR_SHIFTS)))
        mode = str(rs.choice(["step", "train"]))
        ride = str(rs.choice(rides))
        return f"{algo}_{mode}", "forward", dict(algo=algo, mode=mode, steps=1 if mode == "step" else int(rs.integers(1, 4)),
                                                 lr_shift=int(rs.choice(LR_SHIFTS)), fused=bool(ride == "none" and rs.random() < 0.4), ride=ride)
    if group == "log":
        which = str(rs.choice(["td"] + (["tc"] if model.tc else []) + (["mean"] if model.mean else [])))
        restart = bool(model.rst is not None and rs.random() < 0.5)
        if rs.random() < 0.5:
            return "play_log_sweep", "play_log_sweep", dict(lr_shift=int(rs.choice(LR_SHIFTS)), which=which, restart=restart)
        return "backward_train", "backward_train", dict(rounds=int(rs.integers(1, 3)), lr_shift=int(rs.choice(LR_SHIFTS)), which=which,
                                                        restart=restart)
    kind = str(rs.choice(["copy_state", "mask_reset", "set_boards", "set_scores", "owner_reset", "refusal"], p=[0.28, 0.18, 0.14, 0.08, 0.18, 0.14]))
    if kind == "mask_reset":
        return kind, kind, dict(mask=(rs.random(n) < 0.3).astype(np.uint8))
    if kind == "set_boards":
        pool, pick = late_pool(), rs.integers(0, len(late_pool()[0]), n)
        return kind, kind, dict(boards=pool[0][pick], scores=(pool[1][pick] % SAFE_SCORE).astype(np.int32))
    if kind == "set_scores":
        return kind, kind, dict(scores=rs.integers(0, SAFE_SCORE, n).astype(np.int32), on_device=bool(rs.random() < 0.5))
    if kind == "owner_reset":
        owners = [name for name, obj in (("trace", model.trace), ("delay", model.delay), ("restart", model.rst), ("log", model.log),
                                         ("carousel", model.car)) if obj is not None]
        if owners:
            return kind, kind, dict(owner=str(rs.choice(owners)))
        kind = "copy_state"
    if kind == "refusal":
        kinds = ["restart_of_another_size"] if model.rst is not None else []
        kinds += ["carousel_and_restart"] if model.car is not None and model.rst is not None else []
        kinds += ["fused_with_restart"] if model.rst is not None and model.tc is not None else []
        kinds += ["fused_with_carousel"] if model.car is not None else []
        kinds += ["backward_train_with_carousel"] if model.car is not None and model.log is not None else []
        kinds += ["sweep_with_tc_and_mean"] if model.log is not None and model.tc is not None and model.mean is not None else []
        if kinds:
            return kind, kind, dict(kind=str(rs.choice(kinds)))
    return "copy_state", "copy_state", {}


# ================================================================================================ the comparison
def first_difference(got, want):
    """None, or a text on where two values differ: the first differing indices of arrays."""
    if isinstance(want, np.ndarray) or isinstance(got, np.ndarray):
        g, w = np.asarray(got), np.asarray(want)
        if g.shape != w.shape or g.dtype != w.dtype:
            return f"{g.dtype} {list(g.shape)} vs {w.dtype} {list(w.shape)}"
        if np.array_equal(g, w):
            return None
        bad = np.argwhere(g != w)
        i = tuple(bad[0])
        return f"differs at {len(bad)} places, first indices {bad[:4].tolist()}: {g[i]} vs {w[i]}"
    return None if got == want else f"{got} vs {want}"


def compare(got, want, where, what):
    if set(got) != set(want):
        raise Mismatch(f"{where}: {what} {sorted(got)} vs {sorted(want)}")
    for name in want:
        diff = first_difference(got[name], want[name])
        if diff is not None:
            raise Mismatch(f"{where}: {what} {name} {diff}")


def one_case(seed, case, side=None, model_cls=Model, trace=None):
    """Case ``case`` of ``seed``: the model alone (``side`` None), or against ``side(cfg, model)`` -- ``Device``, or another model
    class wrapped by ``against``.  ``trace``: a list that receives the text of every call.  Returns the number of calls."""
    rs = np.random.default_rng([seed, case])
    cfg = Config(rs)
    model = model_cls(cfg)
    other = None if side is None else side(cfg, model)
    tag = f"seed {seed} case {case}: {cfg}"
    bump("cases")
    try:
        if other is not None:
            compare(other.state(), model.state(), f"{tag} before the first call", "state")
        calls = int(rs.integers(12, 31))
        for call in range(calls):
            kind, method, params = draw_call(rs, model)
            text = f"{kind}({digest(params)})"
            where = f"{tag} call {call} {text}"
            bump(kind)
            if trace is not None:
                trace.append(text)
            want = getattr(model, "op_" + method)(**params)
            if not model.in_domain():
                raise OutOfDomain(where)
            if other is not None:
                got = getattr(other, "op_" + method)(**params)
                compare(got, want, where, "output")
                compare(other.state(), model.state(), where, "state")
            if model.mean is not None and not model.mean.is_zero():
                raise Mismatch(f"{where}: the model's mean.sum / mean.count are not all zero after the call")
        for name, count in model.events.items():
            bump("event." + name, count)
        bump("calls", calls)
        return calls
    finally:
        model.close()
        if other is not None:
            other.close()


def against(model_cls):
    """A side of the comparison that is another model (tests: a sabotaged one)."""
    return lambda cfg, model: model_cls(cfg)


def _on_stream(own_streams, fn):
    if not own_streams:
        return fn()
    import torch
    # every case on a fresh NON-DEFAULT (non-blocking) torch stream: nothing in the library may rely on the ordering the null
    # stream gives for free
    with torch.cuda.stream(torch.cuda.Stream()):
        out = fn()
        torch.cuda.current_stream().synchronize()
    return out


def run(budget=120.0, seed=0, cases=None, device=True, own_streams=None) -> str:
    """Fuzz ``seed`` for ``budget`` seconds, or for exactly ``cases`` cases (the run then reproduces); returns the summary line
    (raises Mismatch on the first difference).  ``device`` False: the model alone."""
    if own_streams is None:
        own_streams = os.environ.get("G2048_FUZZ_STREAMS") == "1"
    if device:
        import __graft_entry__ as ge
        ge.build()
    counts.clear()
    t0, case = time.time(), 0
    while (time.time() - t0 < budget) if cases is None else (case < cases):
        try:
            if device:
                _on_stream(own_streams, lambda: one_case(seed, case, Device))
            else:
                one_case(seed, case)
        except OutOfDomain:
            bump("out_of_domain")
        case += 1
    return summary(seed, time.time() - t0, device, own_streams)


def summary(seed, seconds, device=True, own_streams=False):
    ops = {k: v for k, v in sorted(counts.items()) if not k.startswith("event.") and k not in ("cases", "calls", "out_of_domain")}
    events = {k[6:]: v for k, v in sorted(counts.items()) if k.startswith("event.")}
    how = ("every output and every piece of live state of every call bit-exact vs the model" + (", every case on its own stream" if own_streams else "")
           if device else "model alone")
    return (f"ntuple fuzz ok: seed {seed}, {counts.get('cases', 0)} cases ({counts.get('out_of_domain', 0)} left the score range), "
            f"{counts.get('calls', 0)} calls in {seconds:.0f} s, "
            f"operations {ops}, events {events}; {how}")


def main(argv):
    device = "--model-only" not in argv
    argv = [a for a in argv if a != "--model-only"]
    if argv and argv[0] == "--replay":
        seed, case = int(argv[1]), int(argv[2])
        if device:
            import __graft_entry__ as ge
            ge.build()
        trace = []
        counts.clear()
        t0 = time.time()
        try:
            one_case(seed, case, Device if device else None, trace=trace)
        finally:
            print("\n".join(f"call {i} {t}" for i, t in enumerate(trace)))
        print(summary(seed, time.time() - t0, device))
    elif argv and argv[0] == "--cases":
        print(run(seed=int(argv[2]) if len(argv) > 2 else 0, cases=int(argv[1]), device=device))
    else:
        print(run(float(argv[0]) if argv else 120.0, int(argv[1]) if len(argv) > 1 else 0, device=device))


if __name__ == "__main__":
    main(sys.argv[1:])
