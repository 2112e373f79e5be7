"""Shared by the n-tuple adaptive search tests (g2048_ntuple_adaptive_search): the host build of the header's
adaptive search code (tests/host_ntuple_adaptive/adaptive_check.cpp, g++) behind ctypes, the depth-4 reference the CPU and the
GPU tests share (computed once), the composition "depth k + 1 from depth-k values", the 17 boards with 0..16 empty cells and
their mixed schedule, and the per-move composition of an AdaptivePlayer game.  A plain module, like ntuple_deep_helpers."""
import ctypes as C
import types

import numpy as np

import ntuple_ref as ref
import ntuple_search_ref as sref
from analysis_helpers import ONE_LEGAL, TERMINAL
from host_build import Desc, build_host
from ntuple_deep_helpers import cached, compose_depth3, desc_of, near_full, w32_of
from ntuple_helpers import TUPLES_8x4, random_net
from ntuple_search_helpers import PAIR_ONLY

ILLEGAL = ref.ILLEGAL
MAX_DEPTH, SKIPPED = 4, 0xff

# Three crafted near-full boards for the pure-Python reference at depth 4 (2, 2 and 3 legal moves): seconds, where boards of a
# game in progress take minutes
CRAFTED = np.array([[1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 0],
                    [3, 4, 3, 4, 4, 3, 4, 3, 3, 4, 3, 4, 0, 3, 4, 3],
                    [1, 2, 3, 4, 5, 6, 7, 8, 1, 2, 3, 4, 0, 6, 7, 0]], np.uint8)


def crafted_net():
    return cached("adaptive crafted net", lambda: random_net(TUPLES_8x4[:1], 31))


def crafted_reference():
    """(action, value) of CRAFTED at depth 4 by tests/ntuple_search_ref.py, once per process."""
    return cached("adaptive crafted depth 4", lambda: sref.search_batch(CRAFTED, 4, crafted_net()))


def named_boards():
    """The six boards of near_full(2), ONE_LEGAL, PAIR_ONLY and TERMINAL: the boards of the composition at depth 4."""
    return cached("adaptive named", lambda: np.concatenate([near_full(2)[0], ONE_LEGAL, PAIR_ONLY, TERMINAL]))


def compose_next(boards, frac_bits, depth_k):
    """(action, value) at depth k + 1 from the definition and ``depth_k(children uint8 [m, 16]) -> value int64 [m, 4]``, a
    depth-k search of the level-1 children (evaluate's q at k = 0): S_k(child) = the largest legal value, 0 when none is
    legal, the top chance sum and its floor division in Python integers.  ntuple_deep_helpers.compose_depth3 is this at k = 2
    and reads nothing of k: the same code.  Also (the largest item count of a direction, the children without a legal move)."""
    return compose_depth3(boards, frac_bits, depth_k)


def constant(depth):
    return (depth,) * 17


# ------------------------------------------------------------------------------------------------ one board per empty-cell count
MIXED_SCHEDULE = (4, 4, 3, 3, 2, 2, 1, 1, 0, 0, 1, 2, 1, 0, 1, 0, 1)


def empties_boards():
    """uint8 [17, 16]: row E has E empty cells -- PAIR_ONLY (full, two legal moves) with its last E cells cleared."""
    boards = np.repeat(PAIR_ONLY, 17, 0)
    for e in range(17):
        boards[e, 16 - e:] = 0
    assert ((boards == 0).sum(1) == np.arange(17)).all()
    return boards


def rows_at(schedule, boards):
    """({depth: the rows of ``boards`` that ``schedule`` sends to that depth}, the depth of every row as uint8 [n]), from the
    boards' empty cells (mod 32) alone."""
    depths = np.asarray(schedule)[((np.asarray(boards) % 32) == 0).sum(1)]
    return {int(d): np.nonzero(depths == d)[0] for d in np.unique(depths)}, depths.astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the host build
def build_host_adaptive(force=False):
    """g++ build of tests/host_ntuple_adaptive (the device header's adaptive search code compiled for the host; tests only)."""
    return build_host("host_ntuple_adaptive", "adaptive_check.cpp", "libadaptive_check.so", force)


def load_host_adaptive():
    lib = C.CDLL(build_host_adaptive())
    P, u32, u64, D = C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(Desc)
    lib.adaptive_check_root.restype, lib.adaptive_check_root.argtypes = C.c_int, [P, u64, u32, D, P, P, P]
    lib.adaptive_check_split.restype, lib.adaptive_check_split.argtypes = C.c_int, [P, u64, P, D, P, u32, P, P, P, P]
    return lib


def _rows(boards):
    return np.ascontiguousarray(np.asarray(boards, np.uint8).reshape(-1, 16))


def host_root(lib, boards, depth, net):
    """(action uint8 [n], value int64 [n, 4]) of the header's one-thread root on the host, depth 0..4."""
    b, w = _rows(boards), w32_of(net)
    act, val = np.zeros(len(b), np.uint8), np.zeros((len(b), 4), np.int64)
    assert lib.adaptive_check_root(b.ctypes.data, len(b), depth, desc_of(net), w.ctypes.data, act.ctypes.data, val.ctypes.data) == 0
    return act, val


def host_split(lib, boards, schedule, net, P, active=None):
    """(action, value, depth) of the adaptive kernel's split run by P lanes on the host."""
    b, w = _rows(boards), w32_of(net)
    act, val, dep = np.zeros(len(b), np.uint8), np.zeros((len(b), 4), np.int64), np.zeros(len(b), np.uint8)
    sched = np.ascontiguousarray(schedule, np.uint8)
    assert len(sched) == 17
    mask = None if active is None else np.ascontiguousarray(active, np.uint32)
    assert lib.adaptive_check_split(b.ctypes.data, len(b), sched.ctypes.data, desc_of(net), w.ctypes.data, P,
                                    None if mask is None else mask.ctypes.data, act.ctypes.data, val.ctypes.data, dep.ctypes.data) == 0
    return act, val, dep


# ------------------------------------------------------------------------------------------------ the device
def existing_calls(net, d, depth):
    """[(name, NTupleSearch-like (action, value) as numpy)] of the calls that exist for ``depth`` 0..3 on device boards ``d``."""
    def np2(r):
        return r.action.cpu().numpy(), r.value.cpu().numpy()
    if depth == 0:
        return [("evaluate", np2(net.evaluate(d)))]
    calls = []
    if depth <= 2:
        calls.append((f"search({depth})", np2(net.search(d, depth))))
    if depth >= 2:
        calls.append((f"deep_search({depth})", np2(net.deep_search(d, depth))))
    return calls


def composed_depth_4(torch, net, rnet, boards):
    """(b) on the device: depth 4 of ``boards`` from ntuple_deep_search(depth=3) of their children."""
    from ntuple_deep_helpers import dev
    want, _, _ = compose_next(boards, rnet.frac_bits, lambda kids: net.deep_search(dev(torch, kids), 3).value.cpu().numpy())
    return want


def expected_mixed(torch, net, rnet, boards, schedule):
    """(action, value, depth) of ``boards`` under ``schedule`` without the code under test: every board from the existing call
    of its own depth (all of them where two exist, which must agree), depth 4 from the composition."""
    from ntuple_deep_helpers import dev
    from ntuple_search_helpers import assert_search_equal
    rows, depths = rows_at(schedule, boards)
    want = (np.zeros(len(boards), np.uint8), np.zeros((len(boards), 4), np.int64), depths)
    for depth, at in rows.items():
        sub = boards[at]
        if depth == 4:
            a, v = composed_depth_4(torch, net, rnet, sub)
        else:
            calls = existing_calls(net, dev(torch, sub), depth)
            a, v = calls[0][1]
            for name, other in calls[1:]:
                assert_search_equal(other, (a, v), sub, f"{name} vs {calls[0][0]}")
        want[0][at], want[1][at] = a, v
    return want


def adaptive_np(r):
    return tuple(None if t is None else t.cpu().numpy() for t in r)


def dead_rows(got, rows, where=""):
    """Rows ``rows`` of (action, value, ...) are those of a board with no legal move."""
    assert (got[0][rows] == 0).all() and (got[1][rows] == ILLEGAL).all(), f"{where}: a dead board's outputs"


# ------------------------------------------------------------------------------------------------ a game move by move
def composed_game(torch, eng, net, schedule, steps, games=1):
    """``steps`` rounds of ntuple_adaptive_search(active=games left) -> play_step on ``eng`` after a reset, with the side outputs
    play_games keeps: what play_games(player=AdaptivePlayer(net, schedule), max_steps=steps) does, one call at a time."""
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
        eng.ntuple_adaptive_search(net, schedule, out=(act, None, dep), active=left)
        actions.append(act.cpu().numpy().copy())
        depths.append(dep.cpu().numpy().copy())
        eng.play_step(act, games_left=left, hist=hist, moves=moves)
    after = eng.episode_stats()
    return types.SimpleNamespace(actions=np.array(actions), depths=np.array(depths), played=after["episodes"] - before["episodes"],
                                 return_sum=after["return_sum"] - before["return_sum"],
                                 hist=[int(c) for c in hist.view(torch.int64).tolist()], moves=int(moves.view(torch.int64).item()),
                                 left=left.view(torch.int32).cpu().numpy())
