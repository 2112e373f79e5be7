"""Shared by the n-tuple network tests: the host build of the header's n-tuple code (tests/host_ntuple/ntuple_check.cpp,
g++) behind ctypes, the network shapes the tests use, and random weights.  A plain module, like analysis_helpers."""
import ctypes as C
import os
import subprocess

import numpy as np

import ntuple_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_DIR = os.path.join(ROOT, "tests", "host_ntuple")

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
    so, src = os.path.join(HOST_DIR, "libntuple_check.so"), os.path.join(HOST_DIR, "ntuple_check.cpp")
    deps = [src, os.path.join(ROOT, "gym-2048_amd", "csrc", "g2048_device.h")]
    if force or not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", so, src])
    return so


def load_host_ntuple():
    lib = C.CDLL(build_host_ntuple())
    P, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    lib.ntuple_check_evaluate.restype, lib.ntuple_check_evaluate.argtypes = C.c_int, [P, u64, u32, u32, u32, P, P, P, P, P, P, P]
    lib.ntuple_check_values.restype, lib.ntuple_check_values.argtypes = C.c_int, [P, u64, u32, u32, P, P, P]
    lib.ntuple_check_update.restype, lib.ntuple_check_update.argtypes = C.c_int, [P, u64, P, u32, u32, u32, P, P]
    lib.ntuple_check_step.restype, lib.ntuple_check_step.argtypes = C.c_int32, [C.c_int64, u32]
    lib.ntuple_check_sym_cells.restype, lib.ntuple_check_sym_cells.argtypes = None, [P]
    return lib


def _rows(boards):
    return np.ascontiguousarray(np.asarray(boards, np.uint8).reshape(-1, 16))


def _cells(net):
    c = np.zeros((8, 6), np.uint8)
    for t, cells in enumerate(net.tuples):
        c[t, :len(cells)] = cells
    return c


def _w32(net):
    return np.ascontiguousarray(net.weights.astype(np.int32))


def host_evaluate(lib, boards, net):
    b, c, w = _rows(boards), _cells(net), _w32(net)
    n = len(b)
    val, act = np.zeros((n, 4), np.int64), np.zeros(n, np.uint8)
    best, after, av = np.zeros(n, np.int64), np.zeros((n, 16), np.uint8), np.zeros(n, np.int64)
    assert lib.ntuple_check_evaluate(b.ctypes.data, n, len(net.tuples), len(net.tuples[0]), net.frac_bits, c.ctypes.data,
                                     w.ctypes.data, val.ctypes.data, act.ctypes.data, best.ctypes.data, after.ctypes.data,
                                     av.ctypes.data) == 0
    return val, act, best, after, av


def host_values(lib, boards, net):
    b, c, w = _rows(boards), _cells(net), _w32(net)
    v = np.zeros(len(b), np.int64)
    assert lib.ntuple_check_values(b.ctypes.data, len(b), len(net.tuples), len(net.tuples[0]), c.ctypes.data, w.ctypes.data,
                                   v.ctypes.data) == 0
    return v


def host_update(lib, boards, deltas, lr_shift, net):
    """The weights after the update, as int64 [T, 16^L] (``net`` is not modified)."""
    b, c, w = _rows(boards), _cells(net), _w32(net)
    d = np.ascontiguousarray(np.asarray(deltas, np.int64))
    assert lib.ntuple_check_update(b.ctypes.data, len(b), d.ctypes.data, lr_shift, len(net.tuples), len(net.tuples[0]),
                                   c.ctypes.data, w.ctypes.data) == 0
    return w.astype(np.int64)


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
