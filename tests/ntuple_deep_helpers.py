"""Shared by the n-tuple deep search tests (g2048_ntuple_deep_search): the host build of the header's deep
search code (tests/host_ntuple_deep/deep_check.cpp, g++) behind ctypes, the reference results the CPU and the GPU tests share
(computed once), the composition of depth 3 from depth-2 calls, the boards, networks and anchored composition of the value-extremes
tests, and the per-move composition of a DeepPlayer game.  A plain module, like ntuple_helpers."""
import ctypes as C
import types

import numpy as np

import host_build
import ntuple_mixed_ref as mref
import ntuple_ref as ref
import ntuple_search_ref as sref
import ntuple_staged_ref as stref
from analysis_helpers import mid_game
from host_build import Desc, raw_desc
from ntuple_helpers import TUPLES_2x6, TUPLES_8x4, random_net
from ntuple_staged_helpers import LOW_THR

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


# ------------------------------------------------------------------------------------------------ value extremes
INT32_MAX, INT32_MIN = (1 << 31) - 1, -(1 << 31)
# 16 + 16 -> 17, then 17 + 17 -> 18: the largest tiles of a game
MERGING = np.array([[16, 16, 17, 5, 1, 2, 3, 4, 2, 3, 4, 5, 3, 4, 5, 0]], np.uint8)
# a full board of 2^27 .. 2^29 tiles: every move merges, gains of 2^29 .. 2^30 at the root and on the three levels below it,
# none reaching 2^31 at the root (asserted where it is used)
HUGE = np.array([[28, 29, 27, 29, 27, 28, 28, 29, 27, 28, 28, 28, 29, 28, 29, 0]], np.uint8)


def quarter_turn(boards):
    """Every board turned by a quarter (numpy's rot90 of the 4 x 4 cells)."""
    return np.array([np.rot90(b.reshape(4, 4)).reshape(16) for b in np.asarray(boards).reshape(-1, 16)], np.uint8)


TURNED = quarter_turn(HUGE)
# equal to its transpose, tiles 2^27 .. 2^29 with cell (i, j) = 27 + (i + j + 2) mod 3 and one empty cell on the diagonal: no two
# neighbours are equal, so the root moves gain nothing and the tree is small (the reference affords depth 4 in a second),
# while the levels below merge 2^29 tiles; up equals left and right equals down at every depth, so the largest value is shared
SYMMETRIC = np.array([[29, 27, 28, 29, 27, 28, 29, 27, 28, 29, 0, 28, 29, 27, 28, 29]], np.uint8)
# one more board of such tiles: under extreme_net("random", 16, 1) the depth-3 chance sum of its direction 2 is odd and above
# 2^53, 10 052 829 928 238 839 with 10 E = 40, and rounding it to a double moves it across a multiple of 40 (found with the host
# build; the test that uses it asserts this from the exact sum it composes)
SENSITIVE = np.array([[28, 27, 29, 28, 28, 29, 27, 27, 0, 28, 29, 28, 28, 27, 29, 28]], np.uint8)
# HUGE and TURNED with a second empty cell
TWO_EMPTY = np.concatenate([HUGE, TURNED])
TWO_EMPTY[0, 0] = TWO_EMPTY[1, 9] = 0


def cleared(board, cells):
    """``board`` [1, 16] with ``cells`` emptied."""
    out = np.array(board, np.uint8).reshape(1, 16)
    out[0, list(cells)] = 0
    return out


def bound_fill(kind, shape, seed=93):
    """int64 weights at the edge of int32: every entry INT32_MIN ("min"), every entry INT32_MAX ("max"), or one of the two at
    random per entry ("random", a fixed seed)."""
    if kind == "random":
        return np.random.default_rng(seed).choice(np.array([INT32_MIN, INT32_MAX]), size=shape)
    return np.full(shape, {"min": INT32_MIN, "max": INT32_MAX}[kind], np.int64)


def extreme_net(kind, frac_bits, T):
    """The uniform network of the value-extremes tests: TUPLES_8x4[:T] under bound_fill(kind), one per (kind, F, T)."""
    def make():
        net = ref.Net(TUPLES_8x4[:T], frac_bits)
        net.weights[:] = bound_fill(kind, net.weights.shape)
        return net
    return cached(("extreme net", kind, frac_bits, T), make)


def extreme_staged_net():
    """Three stages of TUPLES_8x4 on the low thresholds, one of INT32_MIN / INT32_MAX at random per entry, F = 16."""
    def make():
        net = stref.StagedNet(TUPLES_8x4, LOW_THR[:2], 16)
        net.weights[:] = bound_fill("random", net.weights.shape, 98)
        return net
    return cached("extreme staged net", make)


def extreme_mixed_net():
    """ntuple_mixed_ref.MIX_8 in three stages on the low thresholds, one of INT32_MIN / INT32_MAX at random per entry, F = 16."""
    tuples = mref.MIX_8
    return cached("extreme mixed net", lambda: mref.mixed_net(tuples, LOW_THR[:2], 16, bound_fill("random", (3, mref.n_weights(tuples)), 99)))


def chance_sums(board, depth, net):
    """{d: (gain, empty cells, chance sum before the division)} of the legal root directions, by the reference."""
    out = {}
    for d in range(4):
        a, g, legal = ref.move(ref.plain(board), d)
        if legal:
            out[d] = g, sum(x == 0 for x in a), sum(w * sref.state_value(a[:c] + (e,) + a[c + 1:], depth - 1, net)
                                                    for c in range(16) if a[c] == 0 for e, w in ((1, 9), (2, 1)))
    return out


def values_of(sums, frac_bits):
    """The reference's value[4] from its own chance sums: (g << F) + sum // (10 E), ILLEGAL where the direction has none."""
    return np.array([[(sums[d][0] << frac_bits) + sums[d][2] // (10 * sums[d][1]) if d in sums else sref.ILLEGAL for d in range(4)]], np.int64)


def search_of(sums, frac_bits):
    """(action, value) of one board from chance_sums: the smallest direction of the largest value."""
    value = values_of(sums, frac_bits)
    return np.array([max(sums, key=lambda d: (int(value[0, d]), -d)) if sums else 0], np.uint8), value


_ref_rows, _ref_traces = {}, {}


def reference_rows(boards, depth, net):
    """(action uint8 [n], value int64 [n, 4]) by the pure-Python reference of the network's kind at depth 0..4 (depth 0:
    evaluate's action and q), every (network, depth, board) computed once per process: the CPU and the GPU tests share it.
    ``net`` is one of the cached networks of this module (it is remembered by identity)."""
    boards = np.asarray(boards, np.uint8).reshape(-1, 16)
    act, val = np.zeros(len(boards), np.uint8), np.zeros((len(boards), 4), np.int64)
    for i, b in enumerate(boards):
        key = id(net), depth, b.tobytes()
        if key not in _ref_rows:
            if depth == 0:
                q, a = (ref.evaluate if kind_of(net) == 0 else stref.evaluate)(b, net)[:2]
                _ref_rows[key] = net, a, np.array(q, np.int64)
            else:
                trace = reference_trace(net, depth)
                a, v = sref.search_batch(b, depth, net, trace) if kind_of(net) == 0 else stref.search_batch(b, depth, net, trace)
                _ref_rows[key] = net, a[0], v[0]
        _, act[i], val[i] = _ref_rows[key]
    return act, val


def reference_trace(net, depth):
    """What reference_rows met so far under ``net`` at ``depth``: an ntuple_search_ref.Trace, or the counter dict of
    ntuple_staged_ref (its "stage": {stage: afterstates and leaves read from it}) for a staged or mixed network."""
    return _ref_traces.setdefault((id(net), depth), sref.Trace() if kind_of(net) == 0 else {"memo": {}})


def anchored_search(boards, depth, net, lower, direct_depth, stats):
    """(action, value) of ``boards`` at ``depth`` that owes nothing to the code under test at that depth.  A board with
    direct_depth(board) >= depth comes from reference_rows.  Any other board is composed (compose_depth3: the top chance sum
    and its floor division in Python integers) from ``lower(children, depth - 1) -> (action, value)``, the code under test
    one level down, and of those children a deterministic subset -- the quarter with the fewest empty cells, whose reference
    is the cheapest (the first of equals), and every child without a legal move (by the reference's move) -- is compared with anchored_search of the same children at depth - 1, down to depth 2, which
    is always the reference.  ``stats`` counts "direct" and "composed" boards and the "children", "anchored" and "dead" ones,
    and keeps under "totals" the exact chance sums {(depth, board bytes): [(0, direction, sum, 10 E)]} of the composed boards."""
    from ntuple_search_helpers import assert_search_equal
    boards = np.asarray(boards, np.uint8).reshape(-1, 16)
    act, val = np.zeros(len(boards), np.uint8), np.zeros((len(boards), 4), np.int64)

    def checked(kids):
        got = lower(kids, depth - 1)
        dead = np.array([not any(ref.move(ref.plain(k), d)[2] for d in range(4)) for k in kids])
        few = np.argsort((kids == 0).sum(1), kind="stable")[:(len(kids) + 3) // 4]     # the cheapest references
        pick = np.nonzero(dead | np.isin(np.arange(len(kids)), few))[0]
        want = anchored_search(kids[pick], depth - 1, net, lower, direct_depth, stats)
        assert_search_equal((got[0][pick], got[1][pick]), want, kids[pick], f"anchor at depth {depth - 1}")
        stats["children"] = stats.get("children", 0) + len(kids)
        stats["anchored"] = stats.get("anchored", 0) + len(pick)
        stats["dead"] = stats.get("dead", 0) + int(dead.sum())
        assert 4 * len(pick) >= len(kids) and dead[pick].sum() == dead.sum()
        return got[1]

    for i, b in enumerate(boards):
        if depth <= 2 or direct_depth(b) >= depth:
            stats["direct"] = stats.get("direct", 0) + 1
            a, v = reference_rows(b, depth, net)
        elif not any(ref.move(ref.plain(b), d)[2] for d in range(4)):
            a, v = np.zeros(1, np.uint8), np.full((1, 4), ILLEGAL, np.int64)    # (no children to compose from)
        else:
            stats["composed"] = stats.get("composed", 0) + 1
            (a, v), _, _ = compose_depth3(b, net.frac_bits, checked, stats.setdefault("totals", {}).setdefault((depth, b.tobytes()), []))
        act[i], val[i] = a[0], v[0]
    return act, val


def implied_root_sums(boards, value, frac_bits):
    """A list per board of the root chance sums that ``value`` [n, 4] implies, one per legal direction and exact to within
    10 E <= 150: (value - (gain << F)) * 10 E, gain and E by the reference's move, in Python integers.  Asserts on the way
    that every root gain stays below 2^31 and every legal value below 2^50 in magnitude."""
    out = []
    for b, row in zip(np.asarray(boards).reshape(-1, 16), value):
        sums = []
        for d in range(4):
            a, g, legal = ref.move(ref.plain(b), d)
            assert g < 1 << 31 and legal == (int(row[d]) != ILLEGAL)
            if legal:
                assert abs(int(row[d])) < 1 << 50
                sums.append((int(row[d]) - (g << frac_bits)) * 10 * sum(x == 0 for x in a))
        out.append(sums)
    return out


def fold_sums(board, depth, net):
    """The chance sums one level below the root of a depth-``depth`` search of ``board``, by the reference: what the fold step
    divides.  A list of (sum, 10 E) over every (level-1 child, legal move of it)."""
    out = []
    for d in range(4):
        a, _, legal = ref.move(ref.plain(board), d)
        if legal:
            for c in range(16):
                if a[c] == 0:
                    for e in (1, 2):
                        out += [(s, 10 * E) for _, E, s in chance_sums(a[:c] + (e,) + a[c + 1:], depth - 1, net).values()]
    return out


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
def desc_of(net):
    return host_build.desc_of(net, kind_of(net))


def build_host_deep(force=False):
    """g++ build of tests/host_ntuple_deep (the device header's deep search code compiled for the host; tests only)."""
    return host_build.build_host("host_ntuple_deep", "deep_check.cpp", "libdeep_check.so", force)


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


def compose_depth3(boards, frac_bits, depth2, totals=None):
    """(action, value) at depth 3 from the definition and ``depth2(children uint8 [m, 16]) -> value int64 [m, 4]``, a depth-2
    search: S_2(child) = the largest legal depth-2 value, 0 when none is legal; the chance sum and its floor division in Python
    integers.  Also (the largest item count of a direction, the children without a legal move).  ``totals``: a list that
    receives (board, direction, the exact chance sum, 10 E) of every legal direction."""
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
            if totals is not None:
                totals.append((i, d, total, 10 * empties[i][d]))
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
