"""Shared by the fused n-tuple TD step tests (g2048_ntuple_td_step): the host build of the device header's
fused body in the kernel's lane structure and of the step composed by hand (tests/host_ntuple_td, g++) behind ctypes, the
boards the tests start from, the networks, and the reference: the oracle's step under the pure-Python references' evaluate,
computed once.  A plain module, like ntuple_play_helpers, whose networks, engineered boards and network description it reuses."""
import ctypes as C
import types

import numpy as np

import late_game as lg
import ntuple_play_ref as pref
import ntuple_ref as ref
import ntuple_staged_ref as sref
from host_build import Desc, build_host
from ntuple_helpers import TUPLES_17x4
from ntuple_play_helpers import ENGINEERED_CLOCK, _case, cached, engineered, mixed_case, staged_case, trace_of, uniform_case

K_BLOCK = 256
FIELDS = ("action", "after", "after_value", "best_next", "terminated", "delta")


class TdOut(C.Structure):
    """struct TdOut of td_check.cpp."""
    _fields_ = [(name, C.c_void_p) for name in FIELDS + ("last_records", "counts")]


def build_host_td(force=False):
    """g++ build of tests/host_ntuple_td (the device header's fused TD step compiled for the host; tests only)."""
    return build_host("host_ntuple_td", "td_check.cpp", "libtd_check.so", force)


def load_host_td():
    lib = C.CDLL(build_host_td())
    P, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    for fn in (lib.td_check_fused, lib.td_check_composed):
        fn.restype, fn.argtypes = C.c_int64, [P, u64, u64, u64, u64, u32, C.POINTER(Desc), P, C.POINTER(TdOut)]
    return lib


# ------------------------------------------------------------------------------------------------ the networks
def small_case(seed=304):
    """"17x4" with signed weights in -3..3: V of the four afterstates ties often and q goes below zero."""
    def make():
        rnet = ref.Net(TUPLES_17x4, 10)
        rnet.weights[:] = np.random.default_rng(seed).integers(-3, 4, size=rnet.weights.shape)
        return _case("17x4-small", rnet, rnet.weights.astype(np.int32), TUPLES_17x4, (), 0)
    return cached(("small", seed), make)


CASES = {"small": small_case, "17x4": uniform_case, "staged": staged_case, "mixed": mixed_case}


# ------------------------------------------------------------------------------------------------ the boards
def start_pool():
    """(boards uint8 [160, 16], scores int64 [160]): the 96 engineered late-game boards of ntuple_play_helpers (32 with one
    empty cell, 12 without a legal move, 52 that carry the score deficit) and 64 random mid-game boards -- the boards the
    reference player of "17x4" holds 30 moves after a reset -- with their scores."""
    def make():
        boards, scores, _, _ = engineered()
        mid = trace_of(uniform_case(), 64, 130, 77).after[29]
        mid_boards = mid & 0x1f
        mid_scores = (lg.potential(mid_boards) - lg.record_deficit(mid)) % (1 << 24)
        return np.concatenate([boards, mid_boards]).astype(np.uint8), np.concatenate([scores, mid_scores]).astype(np.int64)
    return cached("td pool", make)


def start_of(n):
    """n boards of the pool and their scores, for any n: board 0 has no legal move (so n = 1 ends an episode on an illegal
    move), board 1 has one empty cell, board 2 is a mid-game board, then the pool in order, repeated."""
    boards, scores = start_pool()
    order = np.concatenate([[32, 0, 96], np.arange(160)])
    pick = order[np.arange(n) % len(order)]
    return boards[pick], scores[pick]


# ------------------------------------------------------------------------------------------------ the reference, once
def reference_steps(case, n, k, max_exp=0):
    """k rounds of evaluate -> step(action, auto-reset) -> evaluate on the oracle from start_of(n) at late_game.BASE_OFFSET and
    ENGINEERED_CLOCK, by ntuple_play_ref's parts: per step the six outputs of the fused call, the records after it, and the
    terminal records; no_move [k, n]: the board had no legal move.  Computed once per argument set, never modified."""
    def make():
        boards, scores = start_of(n)
        o = pref.start_of(n, lg.SEED, lg.BASE_OFFSET, max_exp, boards=boards, scores=scores, clock=ENGINEERED_CLOCK)
        evaluate = (ref if isinstance(case.rnet, ref.Net) else sref).evaluate_batch
        out = types.SimpleNamespace(start=pref.records_of(o.boards, o.score), steps=[], last_records=np.zeros((n, 16), np.uint8),
                                    episodes=0, illegal_ends=0, gain_sum=0, no_move=np.zeros((k, n), bool))
        now = evaluate(o.boards, case.rnet)
        for j in range(k):
            _, action, _, after, after_value = now
            out.no_move[j] = ~lg.legal_moves(o.boards).any(axis=1)
            o.step(action)
            term, illegal = o.terminated != 0, o.illegal != 0
            now = evaluate(o.boards, case.rnet)
            best = now[2]
            out.steps.append(types.SimpleNamespace(action=action.copy(), after=after.copy(), after_value=after_value.copy(), best_next=best.copy(),
                                                   terminated=term.astype(np.uint8), delta=np.where(term, 0, best) - after_value,
                                                   records=pref.records_of(o.boards, o.score)))
            out.last_records[term] = pref.records_of(o.terminal_boards[term], o.last_score[term])
            out.episodes += int(term.sum())
            out.illegal_ends += int((term & illegal).sum())
            out.gain_sum += int(np.where(illegal, 0, o.reward).astype(np.int64).sum())
        return out
    return cached(("td reference", case.name, n, k, max_exp), make)


# ------------------------------------------------------------------------------------------------ the host build
def host_steps(lib, fn, case, records, k, max_exp=0):
    """k consecutive steps of ``fn`` ("fused" or "composed") from ``records`` (not modified) at late_game.BASE_OFFSET, the first
    at transaction ENGINEERED_CLOCK + 1: the fields of reference_steps' result, and ``lanes`` (what every call returned)."""
    rec = np.ascontiguousarray(records, np.uint8).copy()
    n = len(rec)
    out = types.SimpleNamespace(steps=[], last_records=np.zeros((n, 16), np.uint8), lanes=[])
    counts = np.zeros(3, np.uint64)
    call = getattr(lib, "td_check_" + fn)
    for j in range(k):
        s = types.SimpleNamespace(action=np.full(n, 0xee, np.uint8), after=np.full((n, 16), 0xee, np.uint8), after_value=np.zeros(n, np.int64),
                                  best_next=np.zeros(n, np.int64), terminated=np.full(n, 0xee, np.uint8), delta=np.zeros(n, np.int64))
        io = TdOut(*[getattr(s, name).ctypes.data for name in FIELDS], out.last_records.ctypes.data, counts.ctypes.data)
        out.lanes.append(call(rec.ctypes.data, n, lg.SEED, ENGINEERED_CLOCK + 1 + j, lg.BASE_OFFSET, max_exp, C.byref(case.desc),
                              case.w32.ctypes.data, C.byref(io)))
        s.records = rec.copy()
        out.steps.append(s)
    out.episodes, out.illegal_ends, out.gain_sum = (int(c) for c in counts)
    return out


def assert_same_steps(got, want, where):
    """Every output of every step, the records after it, the terminal records and the counts, bit for bit."""
    assert len(got.steps) == len(want.steps)
    for j, (g, w) in enumerate(zip(got.steps, want.steps)):
        for name in FIELDS + ("records",):
            a, b = np.asarray(getattr(g, name)), np.asarray(getattr(w, name))
            assert a.shape == b.shape and np.array_equal(a, b), f"{where}, step {j}: {name} differs on boards {np.argwhere(a != b)[:4].tolist()}"
    assert np.array_equal(got.last_records, want.last_records), f"{where}: last_records"
    for name in ("episodes", "illegal_ends", "gain_sum"):
        assert getattr(got, name) == getattr(want, name), f"{where}: {name} {getattr(got, name)} vs {getattr(want, name)}"
