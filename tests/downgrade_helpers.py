"""Shared by the tile-downgrading tests: the host build of the rule and of the downgraded player's step (tests/host_downgrade,
g++) behind ctypes, the engineered boards with the k each must give, small networks of every shape as reference network +
flat int32 array + what an ``NTupleNet`` needs, and the reference traces, computed once.  A plain module, like
ntuple_play_helpers."""
import ctypes as C
import types

import numpy as np

import downgrade_ref as dref
import ntuple_mixed_ref as mref
import ntuple_play_ref as pref
import ntuple_ref as ref
import ntuple_staged_ref as sref
from host_build import END, Desc, build_host, make_desc
from ntuple_helpers import TUPLES_8x4

MIN_EXP, FLOOR_EXP = 5, 4                                 # the rule of the play tests: at work from the 32 tile on
THR_3 = (sref.stage_mask(16), sref.stage_mask(64))       # S = 3: halving a 64 whose 32 is missing crosses the upper threshold
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def build_host_downgrade(force=False):
    """g++ build of tests/host_downgrade (the device header's rule and downgraded step compiled for the host; tests only)."""
    return build_host("host_downgrade", "downgrade_check.cpp", "libdowngrade_check.so", force)


def load_host_downgrade():
    lib = C.CDLL(build_host_downgrade())
    P, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    lib.downgrade_check_rule.restype = C.c_int
    lib.downgrade_check_rule.argtypes = [P, u64, u32, u32, P, P]
    lib.downgrade_check_play.restype = C.c_int
    lib.downgrade_check_play.argtypes = [P, u64, u64, u64, u64, u32, u32, C.POINTER(Desc), P, u32, u32, P, P, P, P, P, P, P, P, P]
    return lib


# ------------------------------------------------------------------------------------------------ engineered boards
def _board(*tiles):
    return list(tiles) + [0] * (16 - len(tiles))


# name -> (board, min_exp, floor_exp, k): every k worked out by hand from the rule in include/g2048.h
ENGINEERED = {
    "empty": (_board(), 5, 4, 0),
    "m < min_exp": (_board(4, 3, 2, 1, 1, 2), 5, 4, 0),
    "m == min_exp": (_board(5, 3, 2, 1), 5, 4, 4),                              # 4 is missing, one 3
    "full chain": (list(range(16, 0, -1)), 5, 4, 0),                            # 1..16 all there: nothing is missing
    "largest blocked, lower free": (_board(9, 7, 7, 6, 3, 2, 1), 5, 4, 5),      # 8 is missing behind two 7s; 5 is missing, no 4 at all
    "only candidate blocked": (_board(6, 4, 4, 3, 2, 1), 5, 4, 0),              # 5 is missing behind two 4s; 4 is there
    "k == m - 1": (_board(8, 6, 5, 4, 3, 3), 5, 4, 7),
    "k == floor_exp": (_board(7, 6, 5, 3, 2, 2), 5, 4, 4),
    "only floor_exp - 1 missing": (_board(7, 6, 5, 4, 2, 1), 5, 4, 0),          # 3 is missing, below the floor
    "two tiles of m": (_board(8, 8, 5, 4, 3, 1), 5, 4, 7),
    "floor_exp > m": (_board(6, 3, 2, 1), 5, 10, 0),
    "15, 16 and 17": ([17, 16, 15, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1], 15, 4, 14),
    "65536 at min_exp 15": (_board(16, 14, 13, 2, 1), 15, 4, 15),               # becomes a 32768 board
    "floor above the gap": (_board(12, 10, 9, 3), 5, 11, 11),                   # 11 is missing and is the floor; 8..4 are below it
    "min_exp 31": (_board(17, 15, 3), 31, 4, 0),
}


def engineered_rows():
    """(names, boards uint8 [n, 16], min_exp [n], floor_exp [n], k [n])"""
    names = sorted(ENGINEERED)
    cols = list(zip(*(ENGINEERED[name] for name in names)))
    return names, np.array(cols[0], np.uint8), np.array(cols[1]), np.array(cols[2]), np.array(cols[3], np.uint8)


def random_boards(n, seed, high_bits=True):
    """n boards of exponents 0..17, the three high bits of every byte random (what the rule must not read)."""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 18, (n, 16)).astype(np.uint8)
    return b | (rng.integers(0, 8, (n, 16)).astype(np.uint8) << 5) if high_bits else b


def host_rule(lib, boards, min_exp, floor_exp):
    boards = np.ascontiguousarray(boards, np.uint8).reshape(-1, 16)
    out, missing = np.zeros_like(boards), np.zeros(len(boards), np.uint8)
    assert lib.downgrade_check_rule(boards.ctypes.data, len(boards), min_exp, floor_exp, out.ctypes.data, missing.ctypes.data) == 0
    return out, missing


# ------------------------------------------------------------------------------------------------ the networks
def _case(name, rnet, w32, tuples, stages, kind, tuple_len=None):
    return types.SimpleNamespace(name=name, rnet=rnet, w32=np.ascontiguousarray(np.asarray(w32).astype(np.int32).reshape(-1)), tuples=tuples,
                                 stages=stages if stages else None, kind=kind, tuple_len=tuple_len,
                                 desc=make_desc(tuples, rnet.frac_bits, stages, kind, tuple_len))


def small_case(family, T, seed=401):
    """Network T = 1..8 of "uniform" (TUPLES_8x4[:T]), "staged" (the same lists on THR_3) or "mixed" (ntuple_mixed_ref.MIX_8[:T] on
    THR_3: lengths 4, 1, 3, 2, 4, 2, 3, 1): int32 weights within +-2^12, F = 10 -- small against the merge gains, so the games
    run to 64 and 128 tiles inside a hundred moves.  ("mixed", 1) is one list of four cells described with tuple_len 6: its
    list ends early, which is what makes a descriptor mixed."""
    def make():
        rng = np.random.default_rng(seed + 10 * T + {"uniform": 0, "staged": 1, "mixed": 2}[family])
        if family == "uniform":
            rnet = ref.Net(TUPLES_8x4[:T], 10)
            rnet.weights[:] = rng.integers(-(1 << 12), 1 << 12, size=rnet.weights.shape)
            return _case(f"uniform-{T}", rnet, rnet.weights, TUPLES_8x4[:T], (), 0)
        if family == "staged":
            rnet = sref.random_net(TUPLES_8x4[:T], THR_3, seed + 10 * T + 1, lo=-(1 << 12), hi=1 << 12)
            return _case(f"staged-{T}", rnet, rnet.weights, TUPLES_8x4[:T], THR_3, 1)
        tuples = mref.MIX_8[:T]
        flat = rng.integers(-(1 << 12), 1 << 12, size=(3, mref.n_weights(tuples))).astype(np.int32)
        return _case(f"mixed-{T}", mref.mixed_net(tuples, THR_3, 10, flat), flat, tuples, THR_3, 2, 6 if T == 1 else None)
    return cached(("small", family, T, seed), make)


def net_of(g, torch, case):
    """The NTupleNet (``g``: the package) of a case with its weights on the device (cached on the case: one upload per network)."""
    if not hasattr(case, "dev"):
        net = g.NTupleNet(case.tuples, frac_bits=case.rnet.frac_bits, stages=case.stages, mixed=True)
        if case.tuple_len is not None:           # one list described as a mixed network: tuple_len beyond the list's end
            c_net = net._c.net if case.stages else net._c
            for k in range(len(case.tuples[0]), case.tuple_len):
                c_net.cells[0][k] = END
            c_net.tuple_len = case.tuple_len
        net.weights.copy_(torch.from_numpy(case.w32).reshape(net.weights.shape))
        case.dev = net
    return case.dev


# ------------------------------------------------------------------------------------------------ the reference, once
def trace_of(case, n, k_steps, seed, min_exp=MIN_EXP, floor_exp=FLOOR_EXP):
    """The unlimited reference trace of downgraded play of ``case`` on n boards after reset(): computed once, never modified."""
    return cached(("trace", case.name, n, k_steps, seed, min_exp, floor_exp),
                  lambda: dref.unlimited(pref.start_of(n, seed), k_steps, case.rnet, min_exp, floor_exp))


def host_play(lib, case, start_records, seed, t_first, k_steps, min_exp=MIN_EXP, floor_exp=FLOOR_EXP, games_left=None):
    """downgrade_check_play from ``start_records`` (not modified): the fields of ntuple_play_ref.limited's result."""
    rec = np.ascontiguousarray(start_records, np.uint8).copy()
    n = len(rec)
    left = None if games_left is None else np.ascontiguousarray(games_left, np.uint32).copy()
    term, act = np.zeros((k_steps, n), np.uint8), np.zeros((k_steps, n), np.uint8)
    last, eps = np.zeros((n, 16), np.uint8), np.zeros(n, np.uint64)
    sums, hist = np.zeros(3, np.uint64), np.zeros(32, np.uint64)      # return_sum, gain_sum, moves
    assert lib.downgrade_check_play(rec.ctypes.data, n, seed, t_first, 0, k_steps, 0, C.byref(case.desc), case.w32.ctypes.data,
                                    min_exp, floor_exp, None if left is None else left.ctypes.data, term.ctypes.data,
                                    act.ctypes.data, last.ctypes.data, eps.ctypes.data, sums[0:].ctypes.data, sums[1:].ctypes.data,
                                    hist.ctypes.data, sums[2:].ctypes.data) == 0
    return types.SimpleNamespace(records=rec, games_left=left, terminated=term.astype(bool), action=act, last_records=last,
                                 episodes=eps.astype(np.int64), return_sum=int(sums[0]), gain_sum=int(sums[1]), moves=int(sums[2]),
                                 hist=hist)
