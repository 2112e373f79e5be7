"""Shared by the n-tuple deep search tests (g2048_ntuple_deep_search): the host build of the header's deep
search code (tests/host_ntuple_deep/deep_check.cpp, g++) behind ctypes, the reference results the CPU and the GPU tests share
(computed once), the composition of depth 3 from depth-2 calls, and the per-move composition of a DeepPlayer game.  A plain
module, like ntuple_helpers."""
import ctypes as C
import os
import subprocess
import types

import numpy as np

import ntuple_mixed_ref as mref
import ntuple_ref as ref
import ntuple_search_ref as sref
import ntuple_staged_ref as stref
from analysis_helpers import mid_game
from ntuple_helpers import TUPLES_2x6, TUPLES_8x4, random_net
from ntuple_staged_helpers import LOW_THR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_DIR = os.path.join(ROOT, "tests", "host_ntuple_deep")
ILLEGAL = ref.ILLEGAL
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ------------------------------------------------------------------------------------------------ networks
def kind_of(net):
    """0: an ntuple_ref.Net (NtupleShape), 1: a StagedNet of one length (NtupleStagedShape), 2: a mixed one (NtupleMixedShape)."""
    if not hasattr(net, "thr"):
        return 0
    return 2 if len(set(mref.lens(net.tuples))) > 1 else 1


def w32_of(net):
    """The int32 array the device holds: [T, 16^L], [S, T, 16^L] or the compact [S, W] of a mixed network."""
    w = mref.flat_of(net) if kind_of(net) == 2 else net.weights
    return np.ascontiguousarray(np.asarray(w).astype(np.int32))


def mixed_net():
    """A mixed-length reference network, three stages on the low thresholds."""
    tuples = mref.SHAPES["asc"]
    return cached("mixed", lambda: mref.mixed_net(tuples, LOW_THR[:2], 10, mref.random_flat(tuples, 93, 3)))


def staged_net():
    """A 3-stage reference network of two 4-tuples."""
    return cached("staged", lambda: stref.random_net(TUPLES_8x4[:2], LOW_THR[:2], 94))


# The families of tests/test_gpu_ntuple_search_matrix.py: network T of a family has the first T cell lists and the first T
# tables (of every stage) of the family's T = 8 network, full-range random int32, F = 10 -- a launch that took the
# neighbouring instantiation reads the same numbers and computes something else.
FAMILIES = {"uniform": range(1, 9), "staged": range(1, 9), "mixed": range(2, 9)}   # (one list alone cannot be mixed)


def family_net(family, T):
    """Network T of "uniform" (TUPLES_8x4[:T]), "staged" (the same lists, three stages on the low thresholds) or "mixed"
    (ntuple_mixed_ref.MIX_8[:T], three stages): a reference network, one per (family, T)."""
    def make():
        if family == "uniform":
            w = cached("uniform weights", lambda: np.random.default_rng(95).integers(-(1 << 31), 1 << 31, size=(8, 16 ** 4)))
            return ref.Net(TUPLES_8x4[:T], 10, w[:T])
        if family == "staged":
            w = cached("staged weights", lambda: np.random.default_rng(96).integers(-(1 << 31), 1 << 31, size=(3, 8, 16 ** 4)))
            return stref.StagedNet(TUPLES_8x4[:T], LOW_THR[:2], 10, w[:, :T])
        flat = cached("mixed weights", lambda: mref.random_flat(mref.MIX_8, 97, 3))
        tuples = mref.MIX_8[:T]
        return mref.mixed_net(tuples, LOW_THR[:2], 10, flat[:, :mref.n_weights(tuples)])    # the tables lie back to back
    assert 1 <= T <= 8      # ("mixed", 1) is a network of one length: the reference of the neighbour of ("mixed", 2) only
    return cached(("family", family, T), make)


# Two near-full boards of 2s and 4s, in stage 1 of the low thresholds: a merge of two 4s makes the 8 that the second threshold
# asks for, so the leaves of a search lie in two stages (boards of a game in progress hold an 8 everywhere)
LOW_STAGE = np.array([[1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 0, 0], [0, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 0]], np.uint8)


def reference_search(boards, depth, net, trace=None):
    """(action, value) by the pure-Python reference of the network's kind."""
    if kind_of(net) == 0:
        return sref.search_batch(boards, depth, net, trace)
    return stref.search_batch(boards, depth, net, {"memo": {}})


def near_full(max_empty, tuples="1x4"):
    """(boards, reference network, the reference's depth-3 (action, value), its depth-2 (action, value), the depth-3 trace) of
    mid_game(6, 31, max_empty) under random_net(.., 31), computed once: the pure-Python depth-3 search takes seconds."""
    def make():
        boards = mid_game(6, 31, max_empty=max_empty)
        net = random_net({"1x4": TUPLES_8x4[:1], "2x6": TUPLES_2x6}[tuples], 31)
        trace = sref.Trace()
        want3 = sref.search_batch(boards, 3, net, trace)
        return boards, net, want3, sref.search_batch(boards, 2, net), trace
    return cached(("near full", max_empty, tuples), make)


# ------------------------------------------------------------------------------------------------ the device
_nets = {}


def device_net(g, rnet):
    """An NTupleNet on the GPU with the shape and weights of a reference network of any kind (one per reference network)."""
    import torch
    if id(rnet) not in _nets:
        kind = kind_of(rnet)
        net = g.NTupleNet(rnet.tuples, frac_bits=rnet.frac_bits, device="cuda:0", stages=rnet.thr if kind else None, mixed=kind == 2)
        net.weights.copy_(torch.as_tensor(w32_of(rnet)).reshape(net.weights.shape))
        _nets[id(rnet)] = rnet, net
    return _nets[id(rnet)][1]


def dev(torch, a):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda:0")


def to_np(e):
    return tuple(None if t is None else t.cpu().numpy() for t in e)


def dev_u32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to("cuda:0").view(torch.uint32)


def engine_with(g, boards, seed=3):
    """An engine whose records hold ``boards`` with populated score-deficit bits."""
    eng = g.Batched2048(len(boards), seed=seed)
    eng.set_boards(np.asarray(boards) % 32)
    eng.set_scores(np.random.default_rng(1).integers(1, 1 << 24, len(boards)).astype(np.int32))
    return eng


# ------------------------------------------------------------------------------------------------ the host build
class Desc(C.Structure):
    """struct Desc of deep_check.cpp."""
    _fields_ = [("T", C.c_uint32), ("L", C.c_uint32), ("F", C.c_uint32), ("S", C.c_uint32), ("kind", C.c_uint32),
                ("thr", C.c_uint16 * 8), ("cells", (C.c_uint8 * 6) * 8)]


def desc_of(net):
    thr, kind = tuple(getattr(net, "thr", ())), kind_of(net)
    d = Desc(len(net.tuples), max(mref.lens(net.tuples)), net.frac_bits, len(thr) + 1, kind)
    d.thr[:len(thr)] = thr
    cells = mref.cells_of(net.tuples)
    for t in range(8):
        for k in range(6):
            d.cells[t][k] = int(cells[t, k])
    return C.byref(d)


def raw_desc(T, L, F=10, S=1, kind=0):
    """A description by its numbers alone, in or out of range (no cells: for calls that must be refused)."""
    return C.byref(Desc(T, L, F, S, kind))


def build_host_deep(force=False):
    """g++ build of tests/host_ntuple_deep (the device header's deep search code compiled for the host; tests only)."""
    so, src = os.path.join(HOST_DIR, "libdeep_check.so"), os.path.join(HOST_DIR, "deep_check.cpp")
    deps = [src, os.path.join(ROOT, "gym-2048_amd", "csrc", "g2048_device.h")]
    if force or not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", so, src])
    return so


def load_host_deep():
    lib = C.CDLL(build_host_deep())
    P, u32, u64, D = C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(Desc)
    lib.deep_check_root.restype, lib.deep_check_root.argtypes = C.c_int, [P, u64, u32, D, P, P, P]
    lib.deep_check_split.restype, lib.deep_check_split.argtypes = C.c_int, [P, u64, u32, D, P, u32, P, P, P, P, P]
    lib.deep_check_lds_bytes.restype, lib.deep_check_lds_bytes.argtypes = u32, []
    return lib


def _rows(boards):
    return np.ascontiguousarray(np.asarray(boards, np.uint8).reshape(-1, 16))


def host_root(lib, boards, depth, net):
    """(action uint8 [n], value int64 [n, 4]) of ntuple_search_root<depth> on the host, depth 1..3."""
    b, w = _rows(boards), w32_of(net)
    act, val = np.zeros(len(b), np.uint8), np.zeros((len(b), 4), np.int64)
    assert lib.deep_check_root(b.ctypes.data, len(b), depth, desc_of(net), w.ctypes.data, act.ctypes.data, val.ctypes.data) == 0
    return act, val


def host_split(lib, boards, depth, net, P, active=None):
    """((action, value), level-1 items [n], work units [n]) of the deep search kernel's split run by P lanes on the host."""
    b, w = _rows(boards), w32_of(net)
    act, val = np.zeros(len(b), np.uint8), np.zeros((len(b), 4), np.int64)
    items, units = np.zeros(len(b), np.uint32), np.zeros(len(b), np.uint32)
    mask = None if active is None else np.ascontiguousarray(active, np.uint32)
    assert lib.deep_check_split(b.ctypes.data, len(b), depth, desc_of(net), w.ctypes.data, P, None if mask is None else mask.ctypes.data,
                                act.ctypes.data, val.ctypes.data, items.ctypes.data, units.ctypes.data) == 0
    return (act, val), items, units


# ------------------------------------------------------------------------------------------------ depth 3 from depth-2 calls
def children_of(boards):
    """The level-1 chance items of plain boards by the reference's move: a list per (board, direction) of (child board,
    weight), None where the direction is illegal; the gains; the empty cells of the afterstates."""
    items, gains, empties = [], [], []
    for b in np.asarray(boards).reshape(-1, 16):
        per, gs, es = [], [], []
        for d in range(4):
            a, g, legal = ref.move(ref.plain(b), d)
            cells = [c for c in range(16) if a[c] == 0]
            per.append([(a[:c] + (e,) + a[c + 1:], w) for c in cells for e, w in ((1, 9), (2, 1))] if legal else None)
            gs.append(g)
            es.append(len(cells))
        items.append(per), gains.append(gs), empties.append(es)
    return items, gains, empties


def compose_depth3(boards, frac_bits, depth2):
    """(action, value) at depth 3 from the definition and ``depth2(children uint8 [m, 16]) -> value int64 [m, 4]``, a depth-2
    search: S_2(child) = the largest legal depth-2 value, 0 when none is legal; the chance sum and its floor division in Python
    integers.  Also (the largest item count of a direction, the children without a legal move)."""
    items, gains, empties = children_of(boards)
    flat = [child for per in items for lst in per if lst is not None for child, _ in lst]
    val2 = depth2(np.array(flat, np.uint8).reshape(-1, 16))
    legal2 = val2 != ILLEGAL
    s2 = [max(int(v) for v in row[ok]) if ok.any() else 0 for row, ok in zip(val2, legal2)]
    act, val, at = np.zeros(len(items), np.uint8), np.full((len(items), 4), ILLEGAL, np.int64), 0
    widest = 0
    for i, per in enumerate(items):
        for d, lst in enumerate(per):
            if lst is None:
                continue
            total = sum(w * s2[at + j] for j, (_, w) in enumerate(lst))
            at += len(lst)
            widest = max(widest, len(lst))
            val[i, d] = (gains[i][d] << frac_bits) + total // (10 * empties[i][d])
        legal = [d for d in range(4) if per[d] is not None]
        act[i] = max(legal, key=lambda d: (int(val[i, d]), -d)) if legal else 0
    return (act, val), widest, int((~legal2.any(1)).sum())


# ------------------------------------------------------------------------------------------------ a game move by move
def composed_game(torch, eng, net, depth, steps, games=1):
    """``steps`` rounds of ntuple_deep_search(active=games left) -> play_step on ``eng`` after a reset, with the side outputs
    play_games keeps: what play_games(player=DeepPlayer(net, depth), max_steps=steps) does, one call at a time."""
    n, dev = eng.n_envs, eng.device
    eng.reset()
    left = torch.full((n,), games, dtype=torch.int32, device=dev).view(torch.uint32)
    hist = torch.zeros(32, dtype=torch.int64, device=dev).view(torch.uint64)
    moves = torch.zeros(1, dtype=torch.int64, device=dev).view(torch.uint64)
    before = eng.episode_stats()
    act = torch.empty(n, dtype=torch.uint8, device=dev)
    actions = []
    for _ in range(steps):
        eng.ntuple_deep_search(net, depth, out=(act, None), active=left)
        actions.append(act.cpu().numpy().copy())
        eng.play_step(act, games_left=left, hist=hist, moves=moves)
    after = eng.episode_stats()
    return types.SimpleNamespace(actions=np.array(actions), played=after["episodes"] - before["episodes"],
                                 return_sum=after["return_sum"] - before["return_sum"],
                                 hist=[int(c) for c in hist.view(torch.int64).tolist()], moves=int(moves.view(torch.int64).item()),
                                 left=left.view(torch.int32).cpu().numpy())
