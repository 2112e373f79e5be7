"""Shared by the multi-stage n-tuple tests: the host build of the header's staged code (tests/host_ntuple/
ntuple_staged_check.cpp, g++) behind ctypes, the low thresholds that let small boards populate every stage, and the boards
the tests use.  A plain module, like ntuple_helpers."""
import ctypes as C
import os
import subprocess

import numpy as np

import ntuple_staged_ref as sref
from analysis_helpers import mixed_boards
from ntuple_helpers import HOST_DIR, ROOT, _rows

# "has a 4", "has an 8", "has a 16 and an 8": S = 4, and a spawned 4 alone crosses the first threshold
LOW_THR = (sref.stage_mask(4), sref.stage_mask(8), sref.stage_mask(16, 8))
# S = 8 on small boards
THR_8 = (4, 8, 12, 16, 24, 32, 48)


class Desc(C.Structure):
    """struct Desc of ntuple_staged_check.cpp."""
    _fields_ = [("T", C.c_uint32), ("L", C.c_uint32), ("F", C.c_uint32), ("S", C.c_uint32), ("thr", C.c_uint16 * 8),
                ("cells", (C.c_uint8 * 6) * 8)]


def desc_of(net):
    d = Desc(len(net.tuples), len(net.tuples[0]), net.frac_bits, len(net.thr) + 1)
    d.thr[:len(net.thr)] = net.thr
    for t, cells in enumerate(net.tuples):
        for k, c in enumerate(cells):
            d.cells[t][k] = c
    return d


def build_host_ntuple_staged(force=False):
    """g++ build of tests/host_ntuple/ntuple_staged_check.cpp (the device header's staged code compiled for the host)."""
    so, src = os.path.join(HOST_DIR, "libntuple_staged_check.so"), os.path.join(HOST_DIR, "ntuple_staged_check.cpp")
    deps = [src, os.path.join(ROOT, "gym-2048_amd", "csrc", "g2048_device.h")]
    if force or not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", so, src])
    return so


def load_host_ntuple_staged():
    lib = C.CDLL(build_host_ntuple_staged())
    P, u32, u64, D = C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(Desc)
    lib.ntuple_staged_check_mask.restype, lib.ntuple_staged_check_mask.argtypes = None, [P, u64, P]
    lib.ntuple_staged_check_stage.restype, lib.ntuple_staged_check_stage.argtypes = C.c_int, [P, u64, D, P]
    lib.ntuple_staged_check_base.restype, lib.ntuple_staged_check_base.argtypes = C.c_int, [P, u64, D, P]
    lib.ntuple_staged_check_evaluate.restype, lib.ntuple_staged_check_evaluate.argtypes = C.c_int, [P, u64, D, P, P, P, P, P, P]
    lib.ntuple_staged_check_values.restype, lib.ntuple_staged_check_values.argtypes = C.c_int, [P, u64, D, P, P]
    lib.ntuple_staged_check_search.restype, lib.ntuple_staged_check_search.argtypes = C.c_int, [P, u64, u32, D, P, P, P]
    lib.ntuple_staged_check_update.restype, lib.ntuple_staged_check_update.argtypes = C.c_int, [P, u64, P, u32, u32, D, P, P, P]
    lib.ntuple_staged_check_trace_update.restype = C.c_int
    lib.ntuple_staged_check_trace_update.argtypes = [u64, P, u32, u32, D, P, P, P, u32, u32, P, P, u32]
    return lib


def _w32(net):
    return np.ascontiguousarray(net.weights.astype(np.int32))


def host_mask(lib, raw):
    b = _rows(raw)
    out = np.zeros(len(b), np.uint32)
    lib.ntuple_staged_check_mask(b.ctypes.data, len(b), out.ctypes.data)
    return out


def host_stage(lib, raw, net):
    b, out = _rows(raw), np.zeros(len(_rows(raw)), np.uint8)
    assert lib.ntuple_staged_check_stage(b.ctypes.data, len(b), C.byref(desc_of(net)), out.ctypes.data) == 0
    return out


def host_base(lib, boards, net):
    b, out = _rows(boards), np.zeros(len(_rows(boards)), np.uint32)
    assert lib.ntuple_staged_check_base(b.ctypes.data, len(b), C.byref(desc_of(net)), out.ctypes.data) == 0
    return out


def host_evaluate(lib, boards, net):
    b, w = _rows(boards), _w32(net)
    n = len(b)
    val, act = np.zeros((n, 4), np.int64), np.zeros(n, np.uint8)
    best, after, av = np.zeros(n, np.int64), np.zeros((n, 16), np.uint8), np.zeros(n, np.int64)
    assert lib.ntuple_staged_check_evaluate(b.ctypes.data, n, C.byref(desc_of(net)), w.ctypes.data, val.ctypes.data, act.ctypes.data,
                                            best.ctypes.data, after.ctypes.data, av.ctypes.data) == 0
    return val, act, best, after, av


def host_values(lib, boards, net):
    b, w = _rows(boards), _w32(net)
    v = np.zeros(len(b), np.int64)
    assert lib.ntuple_staged_check_values(b.ctypes.data, len(b), C.byref(desc_of(net)), w.ctypes.data, v.ctypes.data) == 0
    return v


def host_search(lib, boards, depth, net):
    b, w = _rows(boards), _w32(net)
    act, val = np.zeros(len(b), np.uint8), np.zeros((len(b), 4), np.int64)
    assert lib.ntuple_staged_check_search(b.ctypes.data, len(b), depth, C.byref(desc_of(net)), w.ctypes.data, act.ctypes.data,
                                          val.ctypes.data) == 0
    return act, val


def _tables(net, tc):
    w = _w32(net)
    err = np.zeros(1, np.int64) if tc is None else np.ascontiguousarray(tc.err.copy())
    mag = np.zeros(1, np.int64) if tc is None else np.ascontiguousarray(tc.mag_i64().copy())
    return w, err, mag


def host_update(lib, boards, deltas, lr_shift, mode, net, tc=None):
    """(weights, err, mag) after the update by the host build, as int64 arrays; mode 0 is the TD(0) update, 1..3 the TC
    update with those phases (``net`` and ``tc`` are not modified)."""
    b, d = _rows(boards), np.ascontiguousarray(np.asarray(deltas, np.int64))
    w, err, mag = _tables(net, tc)
    assert lib.ntuple_staged_check_update(b.ctypes.data, len(b), d.ctypes.data, lr_shift, mode, C.byref(desc_of(net)), w.ctypes.data,
                                          err.ctypes.data, mag.ctypes.data) == 0
    return w.astype(np.int64), err, mag


def host_trace_update(lib, tr, deltas, lr_shift, mode, net, tc=None):
    d = np.ascontiguousarray(np.asarray(deltas, np.int64))
    w, err, mag = _tables(net, tc)
    hist, ln = np.ascontiguousarray(tr.hist), np.ascontiguousarray(tr.len)
    assert lib.ntuple_staged_check_trace_update(tr.n, d.ctypes.data, lr_shift, mode, C.byref(desc_of(net)), w.ctypes.data,
                                                err.ctypes.data, mag.ctypes.data, tr.depth, tr.lam, hist.ctypes.data, ln.ctypes.data,
                                                tr.slot) == 0
    return w.astype(np.int64), err, mag


# ------------------------------------------------------------------------------------------------ boards
def small_boards(n, seed, max_exp=None):
    """Random boards at mixed densities whose largest exponent cycles through 1..5 from board to board (or is ``max_exp``),
    every sixth one a board of the golden trajectories: small tiles, so the low thresholds above put boards into every
    stage, and many boards have a move or a spawn that makes the tile a threshold asks for."""
    rng = np.random.default_rng(seed)
    density = rng.uniform(0.2, 1.0, size=(n, 1))
    top = np.full((n, 1), max_exp) if max_exp else np.arange(n).reshape(n, 1) % 5 + 1
    b = np.where(rng.random((n, 16)) < density, rng.integers(0, 1 << 16, size=(n, 16)) % top + 1, 0).astype(np.uint8)
    b[5::6] = mixed_boards(n, seed)[::2][:len(b[5::6])]
    return b


def depth2_boards(boards, full=3):
    """Boards a pure-Python depth-2 search can afford: the ``full`` boards with the fewest empty cells, and one board of two
    2s whose move merges nothing -- its afterstate holds no 4, so a spawned 4 alone crosses stage_mask(4) below it."""
    boards = np.asarray(boards, np.uint8).reshape(-1, 16)
    two = np.zeros((1, 16), np.uint8)
    two[0, [0, 5]] = 1
    return np.concatenate([boards[np.argsort((boards == 0).sum(1), kind="stable")[:full]], two])


def sparse_boards(k, seed, empties=(5, 8)):
    """k boards of small_boards with 5..8 empty cells: chance nodes of 10..16 items, so the lanes of a depth-2 search that
    split a chance node (items sub, sub + K, ...) each get several."""
    pool = small_boards(25 * k, seed)
    e = (pool == 0).sum(1)
    out = pool[(e >= empties[0]) & (e <= empties[1])][:k]
    assert len(out) == k
    return out


# one 4-tuple (the corner square): the network that keeps the pure-Python depth-2 search of sparse boards affordable
ONE_TUPLE = ((0, 1, 4, 5),)


def with_deficit_bits(boards, seed):
    """Engine-record bytes of plain boards: random score-deficit bits in bits 5..7 of bytes 8..15."""
    raw = np.array(boards, np.uint8).reshape(-1, 16) & 0x1f
    raw[:, 8:] |= (np.random.default_rng(seed).integers(0, 8, size=raw[:, 8:].shape) << 5).astype(np.uint8)
    return raw


def preload_tc(net, seed):
    """A StagedTC with small random accumulators everywhere: rates between 0 and 1 on every look-up."""
    rng = np.random.default_rng(seed)
    mag = rng.integers(0, 1 << 20, size=net.weights.shape).astype(np.uint64)
    err = (rng.integers(-(1 << 20), 1 << 20, size=net.weights.shape) % (mag.astype(np.int64) + 1)).astype(np.int64)
    return sref.StagedTC(None, err, mag)
