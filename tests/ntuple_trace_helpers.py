"""Shared by the n-tuple trace tests: the host build of the header's trace code (tests/host_ntuple_trace/
ntuple_trace_check.cpp, g++) behind ctypes, and synthetic push sequences whose termination masks make the ring wrap, fill
and clear.  A plain module, like ntuple_tc_helpers."""
import ctypes as C
import os
import subprocess

import numpy as np

import ntuple_trace_ref as tref
from analysis_helpers import mixed_boards
from ntuple_helpers import ROOT, _cells, _w32

HOST_DIR = os.path.join(ROOT, "tests", "host_ntuple_trace")
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


def build_host_ntuple_trace(force=False):
    """g++ build of tests/host_ntuple_trace (the device header's trace code compiled for the host; tests only)."""
    so, src = os.path.join(HOST_DIR, "libntuple_trace_check.so"), os.path.join(HOST_DIR, "ntuple_trace_check.cpp")
    deps = [src, os.path.join(ROOT, "gym-2048_amd", "csrc", "g2048_device.h")]
    if force or not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", so, src])
    return so


def load_host_ntuple_trace():
    lib = C.CDLL(build_host_ntuple_trace())
    P, u32, u64, i64 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int64
    lib.ntuple_trace_check_decay.restype, lib.ntuple_trace_check_decay.argtypes = u32, [u32, u32]
    lib.ntuple_trace_check_dk.restype, lib.ntuple_trace_check_dk.argtypes = i64, [i64, u32, u32]
    lib.ntuple_trace_check_push_len.restype, lib.ntuple_trace_check_push_len.argtypes = u32, [u32, u32, u32]
    lib.ntuple_trace_check_len.restype, lib.ntuple_trace_check_len.argtypes = u32, [u32, u32]
    lib.ntuple_trace_check_split.restype, lib.ntuple_trace_check_split.argtypes = u64, [u64, u32, u32]
    lib.ntuple_trace_check_push.restype, lib.ntuple_trace_check_push.argtypes = C.c_int, [P, P, P, P, u64, u32, P, P, u32, P]
    lib.ntuple_trace_check_update.restype = C.c_int
    lib.ntuple_trace_check_update.argtypes = [u64, P, u32, u32, u32, u32, P, P, P, P, u32, u32, P, P, u32]
    return lib


def host_push(lib, tr, after, after_value, best_next, terminated):
    """Push into a copy of the reference trace ``tr`` by the host build: (the new trace, delta)."""
    out = tr.copy()
    out.slot = (tr.slot + 1) % tr.depth
    a = np.ascontiguousarray(np.asarray(after, np.uint8).reshape(tr.n, 16))
    av, bn = np.ascontiguousarray(after_value, np.int64), np.ascontiguousarray(best_next, np.int64)
    term, delta = np.ascontiguousarray(terminated, np.uint8), np.zeros(tr.n, np.int64)
    assert lib.ntuple_trace_check_push(a.ctypes.data, av.ctypes.data, bn.ctypes.data, term.ctypes.data, tr.n, tr.depth,
                                       out.hist.ctypes.data, out.len.ctypes.data, out.slot, delta.ctypes.data) == 0
    return out, delta


def host_trace_update(lib, tr, deltas, lr_shift, mode, net, tc=None):
    """(weights, err, mag) after the update by the host build, as int64 arrays; mode 0 is the TD form, 1..3 the TC form with
    those phases (``net`` and ``tc`` are not modified)."""
    c, w = _cells(net), _w32(net)
    d = np.ascontiguousarray(np.asarray(deltas, np.int64))
    err = np.zeros(1, np.int64) if tc is None else np.ascontiguousarray(tc.err.copy())
    mag = np.zeros(1, np.int64) if tc is None else np.ascontiguousarray(tc.mag_i64().copy())
    hist, ln = np.ascontiguousarray(tr.hist), np.ascontiguousarray(tr.len)
    assert lib.ntuple_trace_check_update(tr.n, d.ctypes.data, lr_shift, mode, len(net.tuples), len(net.tuples[0]), c.ctypes.data,
                                         w.ctypes.data, err.ctypes.data, mag.ctypes.data, tr.depth, tr.lam, hist.ctypes.data,
                                         ln.ctypes.data, tr.slot) == 0
    return w.astype(np.int64), err, mag


def push_inputs(n, pushes, seed, span=1 << 30):
    """``pushes`` synthetic pushes of n boards: a list of (after uint8 [n, 16], after_value, best_next int64 [n], terminated
    uint8 [n]).  Board i terminates at push t when (t + i) % (i % 5 + 3) == 0 -- every board ends several times in twelve
    pushes, at different phases, and board 2 (period 5) has runs of four pushes without an end -- except boards with
    i % 7 == 6, which never end.  Non-zero bytes of ``terminated`` are 1, 2 or 0xff."""
    rng = np.random.default_rng(seed)
    boards = mixed_boards(n * pushes, seed).reshape(pushes, n, 16)
    out = []
    for t in range(pushes):
        i = np.arange(n)
        term = (((t + i) % (i % 5 + 3) == 0) & (i % 7 != 6)).astype(np.uint8) * np.array([1, 2, 0xff], np.uint8)[(t + i) % 3]
        out.append((boards[t], rng.integers(-span, span, n), rng.integers(-span, span, n), term))
    return out


def trace_deltas(n, seed):
    """Mixed-sign deltas for a trace update: small ones whose d_k reaches 0 or sticks at -1, sizes up to beyond the clamp,
    zeros, and the int64 extremes."""
    rng = np.random.default_rng(seed)
    d = rng.integers(-(1 << 20), 1 << 20, n) << rng.integers(0, 22, n)
    d[::9] = 0
    special = [3, -3, 1, -1, (1 << 40) + 1, -(1 << 40) - 1, INT64_MAX, INT64_MIN, 1 << 40, -(1 << 40), 1 << 31, -(1 << 31) - 1, 2, -2]
    d[1::4][:len(special)] = special[:len(d[1::4])]
    return d
