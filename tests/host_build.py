"""Shared by every helper module that loads a host-check program (tests/host_*/*_check.cpp): the one g++ build of such a program
as a shared library, and the ctypes side of the network description those programs take (struct Desc of
tests/host_common/ntuple_host.h).  A plain module, like ntuple_helpers."""
import ctypes as C
import glob
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
HEADERS = (os.path.join(TESTS, "host_common", "*.h"), os.path.join(ROOT, "gym-2048_amd", "csrc", "*.h"))
END = 0xff   # G2048_NTUPLE_END


def stale(target, source):
    """Whether ``target`` is missing, or older than ``source`` or than any header a host-check program can include: those of
    tests/host_common and of gym-2048_amd/csrc."""
    deps = [source] + [h for pattern in HEADERS for h in glob.glob(pattern)]
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


def build_host(subdir, source, library, force=False):
    """g++ build of tests/<subdir>/<source> (the device header's code compiled for the host; tests only) as
    tests/<subdir>/<library>, when it is stale: the path of the library."""
    so, src = os.path.join(TESTS, subdir, library), os.path.join(TESTS, subdir, source)
    if force or stale(so, src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", so, src])
    return so


class Desc(C.Structure):
    """struct Desc of ntuple_host.h: the network of a call; kind 0 / 1 / 2 = the call instantiates NtupleShape (S = 1) /
    NtupleStagedShape (S = 1 included) / NtupleMixedShape."""
    _fields_ = [("T", C.c_uint32), ("L", C.c_uint32), ("F", C.c_uint32), ("S", C.c_uint32), ("kind", C.c_uint32),
                ("thr", C.c_uint16 * 8), ("cells", (C.c_uint8 * 6) * 8)]


def make_desc(tuples, frac_bits, thr, kind, tuple_len=None):
    """The Desc of cell lists, padded with END up to tuple_len (default: the longest list), and stage thresholds."""
    L = max(len(t) for t in tuples) if tuple_len is None else tuple_len
    d = Desc(len(tuples), L, frac_bits, len(thr) + 1, kind)
    d.thr[:len(thr)] = thr
    for t, cells in enumerate(tuples):
        padded = list(cells) + [END] * (L - len(cells))
        d.cells[t][:len(padded)] = padded
    return d


def desc_of(net, kind=None, tuple_len=None):
    """The description of a reference network, by reference: an ntuple_ref.Net, or a network with stage thresholds ``thr``
    (ntuple_staged_ref.StagedNet, ntuple_mixed_ref.mixed_net).  kind None: 0 for the former, 1 for the latter."""
    thr = getattr(net, "thr", None)
    if kind is None:
        kind = 0 if thr is None else 1
    return C.byref(make_desc(net.tuples, net.frac_bits, tuple(thr or ()), kind, tuple_len))


def raw_desc(T, L, F=10, S=1, kind=0):
    """A description by its numbers alone, in or out of range (no cells: for calls that must be refused)."""
    return C.byref(Desc(T, L, F, S, kind))
