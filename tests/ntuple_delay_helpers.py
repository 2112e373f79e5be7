"""Shared by the n-tuple delay tests that run on the CPU: the host build of the header's delay code (tests/host_ntuple_delay,
g++) behind ctypes -- the push and the item loop over NtupleDelayItems on a copy of a reference ring.  A plain module, like
ntuple_helpers."""
import ctypes as C

import numpy as np

from host_build import Desc, build_host, desc_of
from ntuple_mixed_helpers import _tables

ORDERS = {"ascending": 0, "descending": 1, "stride 7": 2}


def load_host_delay():
    lib = C.CDLL(build_host("host_ntuple_delay", "delay_check.cpp", "libdelay_check.so"))
    P, u32, u64, D = C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(Desc)
    lib.delay_check_due.restype, lib.delay_check_due.argtypes = u32, [u32, u32, u32, u32]
    lib.delay_check_push.restype, lib.delay_check_push.argtypes = C.c_int, [P, P, P, P, u64, u32, u32, P, P, P, u32, P]
    lib.delay_check_update.restype, lib.delay_check_update.argtypes = C.c_int, [u64, u32, u32, u32, u32, D, P, P, P, u32, P, P, P, u32]
    return lib


def host_push(lib, dl, after, after_value, best_next, terminated):
    """Push into a copy of the reference ring ``dl`` by the host build: (hist, len, acc, slot, delta)."""
    hist, ln, acc = dl.hist.copy(), dl.len.copy(), np.ascontiguousarray(dl.acc_i64())
    slot = (dl.slot + 1) % dl.depth
    a = np.ascontiguousarray(np.asarray(after, np.uint8).reshape(dl.n, 16))
    av, bn = np.ascontiguousarray(after_value, np.int64), np.ascontiguousarray(best_next, np.int64)
    term, delta = np.ascontiguousarray(terminated, np.uint8), np.zeros(dl.n, np.int64)
    assert lib.delay_check_push(a.ctypes.data, av.ctypes.data, bn.ctypes.data, term.ctypes.data, dl.n, dl.depth, dl.lam, hist.ctypes.data,
                                ln.ctypes.data, acc.ctypes.data, slot, delta.ctypes.data) == 0
    return hist, ln, acc, slot, delta


def host_update(lib, dl, lr_shift, form, mode, order, net, kind, tc=None):
    """(weights, err, mag) as compact int64 arrays after the delay update by the host build (``net``, ``tc`` not modified)."""
    w, err, mag = _tables(net, tc)
    hist, ln, acc = np.ascontiguousarray(dl.hist), np.ascontiguousarray(dl.len), np.ascontiguousarray(dl.acc_i64())
    assert lib.delay_check_update(dl.n, lr_shift, form, mode, order, desc_of(net, kind), w.ctypes.data, err.ctypes.data, mag.ctypes.data,
                                  dl.depth, hist.ctypes.data, ln.ctypes.data, acc.ctypes.data, dl.slot) == 0
    return w.astype(np.int64), err, mag
