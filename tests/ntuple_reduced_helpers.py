"""Shared by the n-tuple reduced search tests (g2048_ntuple_reduced_search): the host build of the header's
reduced search code (tests/host_ntuple_reduced/reduced_check.cpp, g++) behind ctypes, the board sets per depth, a crafted board
with a root tie, the one-level composition with two child depths, the evaluations a search costs counted from the definition,
and the per-move composition of a ReducedPlayer game.  A plain module, like ntuple_adaptive_helpers."""
import ctypes as C
import types

import numpy as np

import ntuple_ref as ref
from analysis_helpers import ONE_LEGAL, TERMINAL, mixed_boards
from host_build import Desc, build_host
from ntuple_adaptive_helpers import CRAFTED, named_boards
from ntuple_deep_helpers import LOW_STAGE, desc_of, w32_of
from ntuple_search_helpers import PAIR_ONLY, WIDE_FANS

ILLEGAL = ref.ILLEGAL
REDUCE4 = (1, 2)

# Equal to its transpose, two empty cells: up and left (and down and right) have mirrored afterstates, and a network looks a
# board up under all eight symmetries, so the two largest root values are the same number -- a root tie at every depth.
TIED = np.array([[1, 2, 3, 4, 2, 5, 6, 7, 3, 6, 0, 1, 4, 7, 1, 0]], np.uint8)
assert np.array_equal(TIED.reshape(4, 4), TIED.reshape(4, 4).T)

STATE_BOARDS = np.concatenate([CRAFTED, PAIR_ONLY, TERMINAL, ONE_LEGAL, TIED])    # against the pure-Python reference


def boards_for(depth):
    """The board sets of tests/test_ntuple_adaptive_host.py per depth, and TIED: late boards at every depth; wide and random boards
    where a one-thread root affords them."""
    if depth == 4:
        return np.concatenate([CRAFTED, LOW_STAGE, PAIR_ONLY, TERMINAL, TIED])
    late = np.concatenate([named_boards(), CRAFTED, LOW_STAGE, TIED])
    if depth == 3:
        return late
    return np.concatenate([late, WIDE_FANS, mixed_boards(24, 51)])


def below(k, R, four):
    """max(k - 1 - R [four], 0): the depth of a child of a chance node of depth k >= 1."""
    return max(k - 1 - (R if four else 0), 0)


# ------------------------------------------------------------------------------------------------ the composition
def compose_reduced(boards, frac_bits, depth, R, state_values):
    """(action, value) at ``depth`` >= 1 from the definition and ``state_values(children uint8 [m, 16], k) -> value int64 [m, 4]``,
    a search of the level-1 children at constant depth k by any call that is not under test at ``depth``: S_k(child) = the largest
    legal value, 0 when none is legal; the 2 children at depth - 1 and the 4 children at max(depth - 1 - R, 0); the top chance
    sum and its floor division in Python integers.  Also the number of children without a legal move."""
    boards = np.asarray(boards, np.uint8).reshape(-1, 16)
    jobs = {}          # k -> list of child tuples
    plan = []
    for i, row in enumerate(boards):
        b = ref.plain(row)
        for d in range(4):
            a, g, legal = ref.move(b, d)
            if not legal:
                continue
            terms = []
            for c in (c for c in range(16) if a[c] == 0):
                for exponent, weight in ((1, 9), (2, 1)):
                    k = below(depth, R, exponent == 2)
                    jobs.setdefault(k, []).append(a[:c] + (exponent,) + a[c + 1:])
                    terms.append((weight, k, len(jobs[k]) - 1))
            plan.append((i, d, g, terms))
    s, dead = {}, 0
    for k, kids in jobs.items():
        v = np.asarray(state_values(np.array(kids, np.uint8), k))
        legal = v != ILLEGAL
        s[k] = [max(int(x) for x in row[m]) if m.any() else 0 for row, m in zip(v, legal)]
        dead += int((~legal).all(1).sum())
    act, val = np.zeros(len(boards), np.uint8), np.full((len(boards), 4), ILLEGAL, np.int64)
    for i, d, g, terms in plan:
        total = sum(w * s[k][at] for w, k, at in terms)
        val[i, d] = (g << frac_bits) + total // (5 * len(terms))
    for i in range(len(boards)):
        legal = [d for d in range(4) if val[i, d] != ILLEGAL]
        act[i] = max(legal, key=lambda d: (val[i, d], -d)) if legal else 0
    return (act, val), dead


# ------------------------------------------------------------------------------------------------ what a search costs
def evaluations(board, depth, R):
    """V look-ups of one board at ``depth`` with the 4 children R plies shallower (R = 0: the adaptive search), counted from the
    definition: a leaf afterstate is one look-up.  Memoised per (board, depth)."""
    memo = {}

    def state(b, k):
        key = (b, k)
        if key not in memo:
            total = 0
            for d in range(4):
                a, _, legal = ref.move(b, d)
                if legal:
                    total += after(a, k)
            memo[key] = total
        return memo[key]

    def after(a, k):
        if k == 0:
            return 1
        total = 0
        for c in (c for c in range(16) if a[c] == 0):
            total += state(a[:c] + (1,) + a[c + 1:], k - 1)
            total += state(a[:c] + (2,) + a[c + 1:], k - 1 if R == 0 else below(k, R, True))
        return total

    return state(ref.plain(board), depth)


# ------------------------------------------------------------------------------------------------ the host build
def build_host_reduced(force=False):
    """g++ build of tests/host_ntuple_reduced (the device header's reduced search code compiled for the host; tests only)."""
    return build_host("host_ntuple_reduced", "reduced_check.cpp", "libreduced_check.so", force)


def load_host_reduced():
    lib = C.CDLL(build_host_reduced())
    P, u32, u64, D = C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(Desc)
    lib.reduced_check_root.restype, lib.reduced_check_root.argtypes = C.c_int, [P, u64, u32, u32, D, P, P, P]
    lib.reduced_check_unit.restype, lib.reduced_check_unit.argtypes = C.c_int, [P, u64, u32, D, P, P]
    lib.reduced_check_split.restype, lib.reduced_check_split.argtypes = C.c_int, [P, u64, P, u32, D, P, u32, P, P, P, P]
    return lib


def _rows(boards):
    return np.ascontiguousarray(np.asarray(boards, np.uint8).reshape(-1, 16))


def host_root(lib, boards, depth, R, net):
    """(action uint8 [n], value int64 [n, 4]) of the definition's recursion over the header's code on the host, depth 0..4."""
    b, w = _rows(boards), w32_of(net)
    act, val = np.zeros(len(b), np.uint8), np.zeros((len(b), 4), np.int64)
    assert lib.reduced_check_root(b.ctypes.data, len(b), depth, R, desc_of(net), w.ctypes.data, act.ctypes.data, val.ctypes.data) == 0
    return act, val


def host_unit(lib, boards, k, net):
    """int64 [n]: S^R_k, k in 0..2, by the tree a lane runs for a work unit."""
    b, w = _rows(boards), w32_of(net)
    val = np.zeros(len(b), np.int64)
    assert lib.reduced_check_unit(b.ctypes.data, len(b), k, desc_of(net), w.ctypes.data, val.ctypes.data) == 0
    return val


def host_split(lib, boards, schedule, R, net, P, active=None):
    """(action, value, depth) of the reduced kernel's split run by P lanes on the host."""
    b, w = _rows(boards), w32_of(net)
    act, val, dep = np.zeros(len(b), np.uint8), np.zeros((len(b), 4), np.int64), np.zeros(len(b), np.uint8)
    sched = np.ascontiguousarray(schedule, np.uint8)
    assert len(sched) == 17
    mask = None if active is None else np.ascontiguousarray(active, np.uint32)
    assert lib.reduced_check_split(b.ctypes.data, len(b), sched.ctypes.data, R, desc_of(net), w.ctypes.data, P,
                                   None if mask is None else mask.ctypes.data, act.ctypes.data, val.ctypes.data, dep.ctypes.data) == 0
    return act, val, dep


# ------------------------------------------------------------------------------------------------ a game move by move
def composed_game(torch, eng, net, schedule, R, steps, games=1):
    """``steps`` rounds of ntuple_reduced_search(active=games left) -> play_step on ``eng`` after a reset, with the side outputs
    play_games keeps: what play_games(player=ReducedPlayer(net, schedule, R), max_steps=steps) does, one call at a time (the way
    ntuple_adaptive_helpers.composed_game composes an AdaptivePlayer game)."""
    n, dev = eng.n_envs, eng.device
    eng.reset()
    left = torch.full((n,), games, dtype=torch.int32, device=dev).view(torch.uint32)
    hist = torch.zeros(32, dtype=torch.int64, device=dev).view(torch.uint64)
    moves = torch.zeros(1, dtype=torch.int64, device=dev).view(torch.uint64)
    before = eng.episode_stats()
    act = torch.empty(n, dtype=torch.uint8, device=dev)
    dep = torch.empty(n, dtype=torch.uint8, device=dev)
    actions, depths = [], []
    for _ in range(steps):
        eng.ntuple_reduced_search(net, schedule, R, out=(act, None, dep), active=left)
        actions.append(act.cpu().numpy().copy())
        depths.append(dep.cpu().numpy().copy())
        eng.play_step(act, games_left=left, hist=hist, moves=moves)
    after = eng.episode_stats()
    return types.SimpleNamespace(actions=np.array(actions), depths=np.array(depths),
                                 played=after["episodes"] - before["episodes"],
                                 return_sum=after["return_sum"] - before["return_sum"],
                                 hist=[int(c) for c in hist.view(torch.int64).tolist()], moves=int(moves.view(torch.int64).item()),
                                 left=left.view(torch.int32).cpu().numpy())
