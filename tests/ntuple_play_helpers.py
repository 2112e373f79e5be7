"""Shared by the n-tuple play tests: the host build of ntuple_play_step inside the fused kernel's loop (tests/host_ntuple_play,
g++) behind ctypes, the networks the tests play -- each as a reference network, a flat int32 weight array and what an
``NTupleNet`` needs -- and the reference traces, computed once.  A plain module, like ntuple_helpers."""
import ctypes as C
import types

import numpy as np

import late_game as lg
import ntuple_mixed_ref as mref
import ntuple_play_ref as pref
import ntuple_ref as ref
import ntuple_staged_ref as sref
from host_build import Desc, build_host, make_desc
from ntuple_helpers import TUPLES_8x4, TUPLES_17x4

THR_3 = (sref.stage_mask(8), sref.stage_mask(32))       # S = 3, low enough that boards cross both inside a short game
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def build_host_play(force=False):
    """g++ build of tests/host_ntuple_play (the device header's fused player compiled for the host; tests only)."""
    return build_host("host_ntuple_play", "ntuple_play_check.cpp", "libntuple_play_check.so", force)


def load_host_play():
    lib = C.CDLL(build_host_play())
    P, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    lib.ntuple_play_check_run.restype = C.c_int
    lib.ntuple_play_check_run.argtypes = [P, u64, u64, u64, u64, u32, u32, C.POINTER(Desc), P, P, P, P, P, P, P, P, P, P]
    return lib


# ------------------------------------------------------------------------------------------------ the networks
def _case(name, rnet, w32, tuples, stages, kind):
    return types.SimpleNamespace(name=name, rnet=rnet, w32=np.ascontiguousarray(w32.reshape(-1)), tuples=tuples,
                                 stages=stages if kind else None, desc=make_desc(tuples, rnet.frac_bits, stages, kind))


def uniform_case(T=5, seed=301, zero=False):
    """The first T of the eight 4-tuples (T = 5: "17x4"): full-range random int32 weights -- a bad player, short games -- or all
    zero, where every V ties and the merge score, then the smallest d, decides."""
    def make():
        tuples = TUPLES_8x4[:T]
        assert T != 5 or tuples == TUPLES_17x4
        rnet = ref.Net(tuples, 10)
        if not zero:
            rnet.weights[:] = np.random.default_rng(seed).integers(-(1 << 31), 1 << 31, size=rnet.weights.shape)
        return _case(f"{T}x4" + ("-zero" if zero else ""), rnet, rnet.weights.astype(np.int32), tuples, (), 0)
    return cached(("uniform", T, seed, zero), make)


def staged_case(seed=302):
    """"17x4" in S = 3 stages ("has an 8", "has a 32"), a different random table per stage."""
    def make():
        rnet = sref.random_net(TUPLES_17x4, THR_3, seed)
        return _case("17x4-S3", rnet, rnet.weights.astype(np.int32), TUPLES_17x4, THR_3, 1)
    return cached(("staged", seed), make)


def mixed_case(seed=303):
    """"4x6+4x4": W = 4 * 16^6 + 4 * 16^4 full-range random int32 weights, too wide to pad for the reference: its rows are
    views of the flat array (ntuple_play_ref.Rows)."""
    def make():
        tuples = mref.PRESET
        flat = mref.random_flat(tuples, seed)
        rnet = sref.StagedNet(tuples, (), 10, [pref.Rows(flat[0], mref.bases(tuples))])
        return _case("4x6+4x4", rnet, flat, tuples, (), 2)
    return cached(("mixed", seed), make)


# ------------------------------------------------------------------------------------------------ the reference, once
def trace_of(case, n, k_steps, seed, board_offset=0, max_exp=0):
    """The unlimited reference trace of ``case`` on n boards after reset(): computed once per argument set, never modified."""
    return cached(("trace", case.name, n, k_steps, seed, board_offset, max_exp),
                  lambda: pref.unlimited(pref.start_of(n, seed, board_offset, max_exp), k_steps, case.rnet))


def budgets(n, seed):
    """A mix of 0, 1, 2 and 2^32 - 1 over n boards, each of them on at least one board."""
    b = np.random.default_rng(seed).choice(np.array([0, 1, 2, pref.NO_LIMIT], np.uint32), n)
    b[:4] = [0, 1, 2, pref.NO_LIMIT]
    return b.astype(np.uint32)


def engineered():
    """(boards, scores, dead, carry): 96 boards of the late-game families -- 32 with one empty cell, 12 full and terminal (rows
    ``dead``) and 52 that carry the score deficit (rows ``carry``, two per deficit) -- played at late_game.BASE_OFFSET."""
    hole, dead, carry = lg.one_hole_family(lg.SEED, per_band=16), lg.full_a_family(lg.SEED, per_band=8), lg.carry_family(lg.SEED)
    boards = np.concatenate([hole.boards[:32], dead.boards[:12], carry.boards[::32]])
    scores = np.concatenate([hole.scores[:32], dead.scores[:12], carry.scores[::32]])
    assert len(boards) == 96
    return boards, scores, slice(32, 44), slice(44, 96)


ENGINEERED_CLOCK = (1 << 32) + 1000


def engineered_trace(case, k_steps):
    """The unlimited reference trace from the engineered boards, with the checks that they reach what they are there for."""
    def make():
        boards, scores, dead, carry = engineered()
        o = pref.start_of(96, lg.SEED, lg.BASE_OFFSET, boards=boards, scores=scores, clock=ENGINEERED_CLOCK)
        tr, k = pref.unlimited(o, k_steps, case.rnet), k_steps
        # a dead board: the action is 0, the move is illegal and the episode ends on it
        assert (tr.action[0, dead] == 0).all() and tr.illegal[0, dead].all() and tr.terminated[0, dead].all()
        assert np.array_equal(tr.terminal[0, dead] & 0x1f, boards[dead])
        # one empty cell: the end test behind the spawn decides both ways
        assert tr.terminated[0, :32].any() and not tr.terminated[0, :32].all() and not tr.illegal[0, :32].any()
        # the carry: the first 4 a board spawns on a deficit of 2^k - 4 carries through the packed field, across the register
        # boundary (bit 12) and, from 2^24 - 4, around to 0
        d = np.stack([lg.record_deficit(tr.start[carry])] + [lg.record_deficit(tr.after[j][carry]) for j in range(k)])
        first = (d[:-1] == d[0]) & ((d[1:] - d[:-1]) % (1 << 24) == 4) & ~tr.terminated[:, carry]
        assert (first & (d[:-1] >= 4092)).any() and (first & ((d[:-1] ^ d[1:]) >> 12 != 0)).any() and (first & (d[1:] == 0)).any()
        return tr
    return cached(("engineered", case.name, k_steps), make)


# ------------------------------------------------------------------------------------------------ the host build
def host_run(lib, case, start_records, seed, t_first, k_steps, games_left=None, board_offset=0, max_exp=0):
    """ntuple_play_check_run from ``start_records`` (not modified): the fields of ntuple_play_ref.limited's result."""
    rec = np.ascontiguousarray(start_records, np.uint8).copy()
    n = len(rec)
    left = None if games_left is None else np.ascontiguousarray(games_left, np.uint32).copy()
    term, act = np.zeros((k_steps, n), np.uint8), np.zeros((k_steps, n), np.uint8)
    last, eps = np.zeros((n, 16), np.uint8), np.zeros(n, np.uint64)
    sums, hist = np.zeros(3, np.uint64), np.zeros(32, np.uint64)      # return_sum, gain_sum, moves
    assert lib.ntuple_play_check_run(rec.ctypes.data, n, seed, t_first, board_offset, k_steps, max_exp, C.byref(case.desc),
                                     case.w32.ctypes.data, None if left is None else left.ctypes.data, term.ctypes.data,
                                     act.ctypes.data, last.ctypes.data, eps.ctypes.data, sums[0:].ctypes.data, sums[1:].ctypes.data,
                                     hist.ctypes.data, sums[2:].ctypes.data) == 0
    return types.SimpleNamespace(records=rec, games_left=left, terminated=term.astype(bool), action=act, last_records=last,
                                 episodes=eps.astype(np.int64), return_sum=int(sums[0]), gain_sum=int(sums[1]), moves=int(sums[2]),
                                 hist=hist)


def assert_same(got, want, where=""):
    """Every field of a run, bit for bit."""
    for name in ("records", "terminated", "action", "last_records", "episodes", "hist"):
        g, w = np.asarray(getattr(got, name)), np.asarray(getattr(want, name))
        assert g.shape == w.shape and np.array_equal(g, w), f"{where}: {name} differs at {np.argwhere(g != w)[:4].tolist()}"
    for name in ("return_sum", "gain_sum", "moves"):
        assert getattr(got, name) == getattr(want, name), f"{where}: {name} {getattr(got, name)} vs {getattr(want, name)}"
    if want.games_left is not None:
        assert np.array_equal(got.games_left, want.games_left), f"{where}: games_left"
