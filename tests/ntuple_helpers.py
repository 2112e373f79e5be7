"""Shared by the n-tuple tests: the one host build of the header's n-tuple code (tests/host_ntuple/ntuple_check.cpp, g++)
behind ctypes -- network, search, TD, TC and trace updates, stages -- the network shapes the tests use, and random weights.
A plain module, like analysis_helpers."""
import ctypes as C

import numpy as np

import ntuple_ref as ref
from host_build import Desc, build_host, desc_of, raw_desc

TUPLES_17x4 = ((0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 4, 5), (1, 2, 5, 6), (5, 6, 9, 10))
TUPLES_4x6 = ((0, 1, 2, 3, 4, 5), (4, 5, 6, 7, 8, 9), (0, 1, 2, 4, 5, 6), (4, 5, 6, 8, 9, 10))
TUPLES_2x6 = TUPLES_4x6[:2]
# T = 8, L = 6: every count and length at its limit
TUPLES_8x6 = TUPLES_4x6 + ((0, 4, 8, 12, 13, 9), (3, 2, 1, 5, 9, 13), (15, 14, 10, 11, 7, 6), (12, 8, 9, 5, 6, 2))

# T = 1..8 at L = 4: network T is the first T lists.  Pairwise different and none a symmetry image of another (as a set of
# cells or as a list), so a look-up that reads the table of another tuple reads other entries: the five of TUPLES_17x4, an
# L, an S and a T shape
TUPLES_8x4 = TUPLES_17x4 + ((0, 1, 2, 4), (0, 1, 5, 6), (0, 1, 2, 5))
# L = 1..6 at T = 3: prefixes of the first three 6-cell lists
TUPLES_3xL = {L: tuple(t[:L] for t in TUPLES_4x6[:3]) for L in range(1, 7)}


def symmetry_images(cells):
    """The eight images of a cell list under the board's symmetries, by the reference's own permutations."""
    out = []
    for perm in ref._sym_perms():
        where = {c: k for k, c in enumerate(perm)}      # perm[k] = the cell that lands on k
        out.append(tuple(where[c] for c in cells))
    return out


def build_host_ntuple(force=False):
    """g++ build of tests/host_ntuple (the device header's n-tuple code compiled for the host; tests only)."""
    return build_host("host_ntuple", "ntuple_check.cpp", "libntuple_check.so", force)


def load_host_ntuple():
    lib = C.CDLL(build_host_ntuple())
    P, u32, u64, i64, D = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int64, C.POINTER(Desc)
    for name, restype, argtypes in (
            ("step", C.c_int32, [i64, u32]), ("sym_cells", None, [P]), ("floor_div", i64, [i64, i64]),
            ("tc_rate", u32, [i64, u64]), ("tc_step", C.c_int32, [i64, u32, u32]),
            ("decay", u32, [u32, u32]), ("dk", i64, [i64, u32, u32]), ("push_len", u32, [u32, u32, u32]), ("len", u32, [u32, u32]),
            ("split", u64, [u64, u32, u32]),
            ("mask", None, [P, u64, P]), ("stage", C.c_int, [P, u64, D, P]), ("base", C.c_int, [P, u64, D, P]),
            ("evaluate", C.c_int, [P, u64, D, P, P, P, P, P, P]), ("values", C.c_int, [P, u64, D, P, P]),
            ("search", C.c_int, [P, u64, u32, D, P, P, P]), ("chance_split", C.c_int, [P, u64, u32, D, P, u32, P]),
            ("update", C.c_int, [P, u64, P, u32, u32, D, P, P, P]), ("tc_update", C.c_int, [P, u64, P, u32, u32, D, P, P, P]),
            ("push", C.c_int, [P, P, P, P, u64, u32, P, P, u32, P]),
            ("trace_update", C.c_int, [u64, P, u32, u32, D, P, P, P, u32, u32, P, P, u32])):
        f = getattr(lib, "ntuple_check_" + name)
        f.restype, f.argtypes = restype, argtypes
    return lib


def _rows(boards):
    return np.ascontiguousarray(np.asarray(boards, np.uint8).reshape(-1, 16))


def _w32(net):
    return np.ascontiguousarray(net.weights.astype(np.int32))


def _tables(net, tc):
    w = _w32(net)
    err = np.zeros(1, np.int64) if tc is None else np.ascontiguousarray(tc.err.copy())
    mag = np.zeros(1, np.int64) if tc is None else np.ascontiguousarray(tc.mag_i64().copy())
    return w, err, mag


def host_mask(lib, raw):
    b = _rows(raw)
    out = np.zeros(len(b), np.uint32)
    lib.ntuple_check_mask(b.ctypes.data, len(b), out.ctypes.data)
    return out


def host_stage(lib, raw, net):
    b, out = _rows(raw), np.zeros(len(_rows(raw)), np.uint8)
    assert lib.ntuple_check_stage(b.ctypes.data, len(b), desc_of(net), out.ctypes.data) == 0
    return out


def host_base(lib, boards, net):
    b, out = _rows(boards), np.zeros(len(_rows(boards)), np.uint32)
    assert lib.ntuple_check_base(b.ctypes.data, len(b), desc_of(net), out.ctypes.data) == 0
    return out


def host_evaluate(lib, boards, net):
    b, w = _rows(boards), _w32(net)
    n = len(b)
    val, act = np.zeros((n, 4), np.int64), np.zeros(n, np.uint8)
    best, after, av = np.zeros(n, np.int64), np.zeros((n, 16), np.uint8), np.zeros(n, np.int64)
    assert lib.ntuple_check_evaluate(b.ctypes.data, n, desc_of(net), w.ctypes.data, val.ctypes.data, act.ctypes.data,
                                     best.ctypes.data, after.ctypes.data, av.ctypes.data) == 0
    return val, act, best, after, av


def host_values(lib, boards, net):
    b, w = _rows(boards), _w32(net)
    v = np.zeros(len(b), np.int64)
    assert lib.ntuple_check_values(b.ctypes.data, len(b), desc_of(net), w.ctypes.data, v.ctypes.data) == 0
    return v


def host_search(lib, boards, depth, net):
    """(action uint8 [n], value int64 [n, 4]) of ntuple_search_root on the host."""
    b, w = _rows(boards), _w32(net)
    act, val = np.zeros(len(b), np.uint8), np.zeros((len(b), 4), np.int64)
    assert lib.ntuple_check_search(b.ctypes.data, len(b), depth, desc_of(net), w.ctypes.data, act.ctypes.data, val.ctypes.data) == 0
    return act, val


def host_split(lib, boards, depth, net, K):
    """int64 [n, 4]: the chance sums of the four afterstates, summed over K lanes' parts (0 where the move is illegal)."""
    b, w = _rows(boards), _w32(net)
    out = np.zeros((len(b), 4), np.int64)
    assert lib.ntuple_check_chance_split(b.ctypes.data, len(b), depth, desc_of(net), w.ctypes.data, K, out.ctypes.data) == 0
    return out


def host_update(lib, boards, deltas, lr_shift, mode, net, tc=None):
    """(weights, err, mag) after the one-step update by the host build, as int64 arrays; mode 0 is the TD(0) update, 1..3 the
    TC update with those phases (``net`` and ``tc`` are not modified)."""
    b, d = _rows(boards), np.ascontiguousarray(np.asarray(deltas, np.int64))
    w, err, mag = _tables(net, tc)
    assert lib.ntuple_check_update(b.ctypes.data, len(b), d.ctypes.data, lr_shift, mode, desc_of(net), w.ctypes.data,
                                   err.ctypes.data, mag.ctypes.data) == 0
    return w.astype(np.int64), err, mag


def host_push(lib, tr, after, after_value, best_next, terminated):
    """Push into a copy of the reference trace ``tr`` by the host build: (the new trace, delta)."""
    out = tr.copy()
    out.slot = (tr.slot + 1) % tr.depth
    a = np.ascontiguousarray(np.asarray(after, np.uint8).reshape(tr.n, 16))
    av, bn = np.ascontiguousarray(after_value, np.int64), np.ascontiguousarray(best_next, np.int64)
    term, delta = np.ascontiguousarray(terminated, np.uint8), np.zeros(tr.n, np.int64)
    assert lib.ntuple_check_push(a.ctypes.data, av.ctypes.data, bn.ctypes.data, term.ctypes.data, tr.n, tr.depth,
                                 out.hist.ctypes.data, out.len.ctypes.data, out.slot, delta.ctypes.data) == 0
    return out, delta


def host_trace_update(lib, tr, deltas, lr_shift, mode, net, tc=None):
    """(weights, err, mag) after the trace update by the host build, as int64 arrays; mode as in host_update."""
    d = np.ascontiguousarray(np.asarray(deltas, np.int64))
    w, err, mag = _tables(net, tc)
    hist, ln = np.ascontiguousarray(tr.hist), np.ascontiguousarray(tr.len)
    assert lib.ntuple_check_trace_update(tr.n, d.ctypes.data, lr_shift, mode, desc_of(net), w.ctypes.data, err.ctypes.data,
                                         mag.ctypes.data, tr.depth, tr.lam, hist.ctypes.data, ln.ctypes.data, tr.slot) == 0
    return w.astype(np.int64), err, mag


def random_net(tuples, seed, frac_bits=10, lo=-(1 << 31), hi=1 << 31):
    """A reference network whose weights are uniform in [lo, hi)."""
    net = ref.Net(tuples, frac_bits)
    net.weights[:] = np.random.default_rng(seed).integers(lo, hi, size=net.weights.shape)
    return net


EVAL_NAMES = ("value", "action", "best", "after", "after_value")


def assert_eval_equal(got, want, boards=None, where=""):
    for name, g, w in zip(EVAL_NAMES, got, want):
        g, w = np.asarray(g), np.asarray(w)
        bad = np.nonzero((g.reshape(len(g), -1) != w.reshape(len(w), -1)).any(1))[0]
        assert len(bad) == 0, (f"{where}: {name} differs on {len(bad)} boards, first row {bad[0]}"
                               f"{'' if boards is None else ' ' + str(np.asarray(boards).reshape(-1, 16)[bad[0]].tolist())}: "
                               f"{g[bad[0]].tolist()} vs {w[bad[0]].tolist()}")
