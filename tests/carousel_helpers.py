"""Shared by the carousel tests: the host build of the header's carousel code (tests/host_carousel/carousel_check.cpp, g++)
behind ctypes, its stand-alone sanitizer driver, record builders, and the comparison of a device Carousel with the reference
(tests/carousel_ref.py).  A plain module, like ntuple_helpers."""
import ctypes as C
import os
import subprocess

import numpy as np

import carousel_ref as cref
from host_build import TESTS, build_host, stale

HOST_DIR = os.path.join(TESTS, "host_carousel")
SRC = os.path.join(HOST_DIR, "carousel_check.cpp")


def build_host_carousel(force=False):
    """g++ build of tests/host_carousel as a shared library (the device header's carousel code compiled for the host)."""
    return build_host("host_carousel", "carousel_check.cpp", "libcarousel_check.so", force)


def build_sanitized_driver(force=False):
    """The same file as a stand-alone program (its own main) under AddressSanitizer and UBSan."""
    exe = os.path.join(HOST_DIR, "carousel_driver_asan")
    if force or stale(exe, SRC):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-DCAROUSEL_CHECK_MAIN", "-Wall", "-Wno-unknown-pragmas", "-o", exe, SRC])
    return exe


def load_host_carousel():
    lib = C.CDLL(build_host_carousel())
    P, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    for name, restype, argtypes in (
            ("stage", C.c_int, [P, u64, u32, P, P]), ("top", u32, [P, u32]), ("choice", u32, [u32, u32, u32]),
            ("fill", u32, [u64, u32]), ("sample", u32, [u32, u32, u32, u32, u64]), ("seen", u32, [u32, u32]),
            ("is_entry", C.c_int, [u32]), ("slot", C.c_int64, [u64, u32, u32, u32]), ("range", u64, [u64, u32, u32]),
            ("step", C.c_int, [P, u64, u64, P, u32, P, u32, u64, P, P, P, P, u64])):
        f = getattr(lib, "carousel_check_" + name)
        f.restype, f.argtypes = restype, argtypes
    return lib


def host_step(lib, car, records, terminated, index_offset=0, per=256):
    """The carousel step by the host build, in place on ``records`` and on the reference state ``car``."""
    thr = np.zeros(7, np.uint16)
    thr[:len(car.thr)] = car.thr
    count = np.array(car.count, np.uint64)
    term = np.ascontiguousarray(terminated, np.uint8)
    assert records.flags.c_contiguous and records.dtype == np.uint8
    assert lib.carousel_check_step(records.ctypes.data, car.n, index_offset, term.ctypes.data, car.n_stages, thr.ctypes.data,
                                   car.capacity, car.seed, car.pool.ctypes.data, count.ctypes.data, car.seen.ctypes.data,
                                   car.episodes.ctypes.data, per) == 0
    car.count = [int(c) for c in count]
    return records


# ---------------------------------------------------------------------------------------------------- records
def record(cells, spare=0):
    """A 16-byte engine record: ``cells`` (16 exponents 0..31) with ``spare`` (24 bits) in bits 5..7 of bytes 8..15 -- any
    value will do for the carousel, which copies records verbatim."""
    rec = np.array(cells, np.uint8) & 0x1f
    for k in range(24):
        rec[8 + k // 3] |= ((spare >> k) & 1) << (5 + k % 3)
    return rec


def board_with(*exps):
    """16 cells holding the given exponents, the rest empty."""
    cells = [0] * 16
    cells[:len(exps)] = exps
    return cells


def assert_state_equal(dev, car, records_dev, records_ref, where=""):
    """The device Carousel ``dev`` and its records equal the reference ``car`` and its records, byte for byte."""
    for name, got, want in (("records", records_dev.cpu().numpy(), records_ref), ("pool", dev.pool.cpu().numpy(), car.pool),
                            ("count", dev.count.cpu().numpy(), car.count_i64()), ("seen", dev.seen.cpu().numpy(), car.seen),
                            ("episodes", dev.episodes.cpu().numpy().view(np.uint32), car.episodes)):
        if not np.array_equal(got, want):
            bad = np.nonzero((np.asarray(got).reshape(len(got), -1) != np.asarray(want).reshape(len(want), -1)).any(1))[0]
            raise AssertionError(f"{where}: {name} differs in {len(bad)} rows, first {bad[0]}: "
                                 f"{np.asarray(got)[bad[0]].tolist()} vs {np.asarray(want)[bad[0]].tolist()}")


def load_into(dev, car):
    """Copy the reference state into the device Carousel."""
    dev.load_state_dict({"stages": car.thr, "capacity": car.capacity, "seed": car.seed, "pool": car.pool,
                         "count": car.count_i64(), "seen": car.seen, "episodes": car.episodes.view(np.int32)})


__all__ = ["cref"]
