"""Shared by the midpoint-restart tests (g2048_restart_step, g2048_ntuple_play_log_restart): the host build of
the device header's restart_board in the kernel's lane structure (tests/host_restart, g++) behind ctypes, the stand-alone
sanitizer build of the same file, and the comparison of a restart state with the reference's (tests/restart_ref.py).  A plain
module, like ntuple_log_helpers."""
import ctypes as C
import os
import subprocess

import numpy as np

from host_build import TESTS, build_host, stale

K_BLOCK = 256
FIELDS = ("snap", "pos", "start", "restarts")


class HostRestart(C.Structure):
    """struct HostRestart of restart_check.cpp."""
    _fields_ = [("stride_log2", C.c_uint32), ("capacity", C.c_uint32), ("min_span", C.c_uint32), ("max_restarts", C.c_uint32),
                ("snap", C.c_void_p), ("pos", C.c_void_p), ("start", C.c_void_p), ("restarts", C.c_void_p)]


def load_host_restart():
    lib = C.CDLL(build_host("host_restart", "restart_check.cpp", "librestart_check.so"))
    lib.restart_check_step.restype = C.c_int64
    lib.restart_check_step.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(HostRestart), C.c_uint32]
    return lib


def build_sanitized():
    """The stand-alone program of restart_check.cpp (its own main) under -fsanitize=address,undefined: the path of the
    executable.  It is run directly, never loaded into Python.  The runtimes are linked into the program, so that it starts
    whatever else the process environment has the loader bring in first."""
    d = os.path.join(TESTS, "host_restart")
    exe, src = os.path.join(d, "restart_check_asan"), os.path.join(d, "restart_check.cpp")
    if stale(exe, src):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-DRESTART_CHECK_MAIN", "-o", exe, src])
    return exe


def host_restart_of(st):
    """(HostRestart over the arrays of a restart_ref.State, which must stay alive and contiguous)."""
    r = st.rule
    for name in FIELDS:
        assert getattr(st, name).flags["C_CONTIGUOUS"]
    return HostRestart(r.k, r.C, r.min_span, r.max_restarts, st.snap.ctypes.data, st.pos.ctypes.data, st.start.ctypes.data,
                       st.restarts.ctypes.data)


def assert_state_equal(got, want, where):
    """``got``: anything with snap / pos / start / restarts as arrays (uint32 or the int32 of a torch tensor); ``want``: a State."""
    for name in FIELDS:
        g, w = np.asarray(getattr(got, name)), getattr(want, name)
        g = g.view(np.uint32) if g.dtype == np.int32 else g
        assert g.shape == w.shape and g.dtype == w.dtype, f"{where}: {name} is {g.dtype} {g.shape}"
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError(f"{where}: {name} differs at {len(bad)} places, first {bad[:4].tolist()}")
