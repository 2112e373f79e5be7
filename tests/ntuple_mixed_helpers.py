"""Shared by the mixed-length n-tuple tests: the host build of the header's mixed code (tests/host_ntuple_mixed, g++) behind
ctypes, and the boards the tests use.  A plain module, like ntuple_helpers."""
import ctypes as C
import types

import numpy as np

import host_build
import ntuple_mixed_ref as mref
import ntuple_staged_ref as sref
import ntuple_trace_ref as tref
from analysis_helpers import ONE_LEGAL, TERMINAL, mid_game, mixed_boards
from host_build import Desc
from ntuple_search_helpers import PAIR_ONLY
from ntuple_staged_helpers import small_boards
from ntuple_tc_helpers import preload
from ntuple_trace_helpers import push_inputs

TIE = np.array([[0] * 5 + [3] + [0] * 10], np.uint8)    # the four afterstates are images of one another: four equal values
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def boards_67():
    """The 64 boards of tests/test_gpu_ntuple_shapes.py -- 60 mixed boards, the tie board, PAIR_ONLY, ONE_LEGAL and TERMINAL
    -- and the three edge boards: [0]*16 reads entry 0 of every table, [15]*16 and [17]*16 the last."""
    return cached("boards", lambda: np.concatenate([mixed_boards(60, 81), TIE, PAIR_ONLY, ONE_LEGAL, TERMINAL, mref.edge_boards()]))


def near_full_12():
    """The 12 near-full boards of tests/test_gpu_ntuple_shapes.py, for depth 2."""
    return cached("near full", lambda: np.concatenate([mid_game(10, 82, max_empty=2), PAIR_ONLY, TERMINAL]))


def desc_of(net, tuple_len=None):
    """The description of a reference network (ntuple_mixed_ref.mixed_net): END-padded lists up to tuple_len, the
    NtupleMixedShape code."""
    return host_build.desc_of(net, 2, tuple_len)


def build_host_mixed(force=False):
    return host_build.build_host("host_ntuple_mixed", "ntuple_mixed_check.cpp", "libntuple_mixed_check.so", force)


def load_host_mixed():
    lib = C.CDLL(build_host_mixed())
    P, u32, u64, D = C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(Desc)
    for name, argtypes in (("shape", [D, P, P, P, P]), ("offsets", [P, u64, D, P]), ("values", [P, u64, D, P, P]),
                           ("evaluate", [P, u64, D, P, P, P, P, P, P]), ("search", [P, u64, u32, D, P, P, P]),
                           ("update", [P, u64, P, u32, u32, D, P, P, P]),
                           ("trace_update", [u64, P, u32, u32, D, P, P, P, u32, u32, P, P, u32])):
        f = getattr(lib, "ntuple_mixed_check_" + name)
        f.restype, f.argtypes = C.c_int, argtypes
    return lib


def _rows(boards):
    return np.ascontiguousarray(np.asarray(boards, np.uint8).reshape(-1, 16))


def _w32(net):
    """The compact int32 [S * W] array of a reference network: what the device holds."""
    return np.ascontiguousarray(mref.flat_of(net).astype(np.int32).reshape(-1))


def host_shape(lib, net, tuple_len=None):
    mixed, W = C.c_uint32(), C.c_uint32()
    ln, base = np.zeros(8, np.uint32), np.zeros(8, np.uint32)
    assert lib.ntuple_mixed_check_shape(desc_of(net, tuple_len), C.addressof(mixed), C.addressof(W), ln.ctypes.data, base.ctypes.data) == 0
    T = len(net.tuples)
    return mixed.value, W.value, ln[:T].tolist(), base[:T].tolist()


def host_offsets(lib, boards, net, tuple_len=None):
    b = _rows(boards)
    out = np.zeros((len(b), 8 * len(net.tuples)), np.uint32)
    assert lib.ntuple_mixed_check_offsets(b.ctypes.data, len(b), desc_of(net, tuple_len), out.ctypes.data) == 0
    return out


def host_values(lib, boards, net):
    b, w = _rows(boards), _w32(net)
    v = np.zeros(len(b), np.int64)
    assert lib.ntuple_mixed_check_values(b.ctypes.data, len(b), desc_of(net), w.ctypes.data, v.ctypes.data) == 0
    return v


def host_evaluate(lib, boards, net):
    b, w = _rows(boards), _w32(net)
    n = len(b)
    val, act = np.zeros((n, 4), np.int64), np.zeros(n, np.uint8)
    best, after, av = np.zeros(n, np.int64), np.zeros((n, 16), np.uint8), np.zeros(n, np.int64)
    assert lib.ntuple_mixed_check_evaluate(b.ctypes.data, n, desc_of(net), w.ctypes.data, val.ctypes.data, act.ctypes.data,
                                           best.ctypes.data, after.ctypes.data, av.ctypes.data) == 0
    return val, act, best, after, av


def host_search(lib, boards, depth, net):
    b, w = _rows(boards), _w32(net)
    act, val = np.zeros(len(b), np.uint8), np.zeros((len(b), 4), np.int64)
    assert lib.ntuple_mixed_check_search(b.ctypes.data, len(b), depth, desc_of(net), w.ctypes.data, act.ctypes.data, val.ctypes.data) == 0
    return act, val


def _tables(net, tc):
    w = _w32(net)
    if tc is None:
        return w, np.zeros(1, np.int64), np.zeros(1, np.int64)
    err, mag = mref.tc_flat(tc, net)
    return w, np.ascontiguousarray(err.reshape(-1)), np.ascontiguousarray(mag.reshape(-1))


def host_update(lib, boards, deltas, lr_shift, mode, net, tc=None):
    """(weights, err, mag) as compact int64 arrays after the one-step update by the host build; mode 0 is the TD(0) update,
    1..3 the TC update with those phases (``net`` and ``tc`` are not modified)."""
    b, d = _rows(boards), np.ascontiguousarray(np.asarray(deltas, np.int64))
    w, err, mag = _tables(net, tc)
    assert lib.ntuple_mixed_check_update(b.ctypes.data, len(b), d.ctypes.data, lr_shift, mode, desc_of(net), w.ctypes.data,
                                         err.ctypes.data, mag.ctypes.data) == 0
    return w.astype(np.int64), err, mag


def host_trace_update(lib, tr, deltas, lr_shift, mode, net, tc=None):
    d = np.ascontiguousarray(np.asarray(deltas, np.int64))
    w, err, mag = _tables(net, tc)
    hist, ln = np.ascontiguousarray(tr.hist), np.ascontiguousarray(tr.len)
    assert lib.ntuple_mixed_check_trace_update(tr.n, d.ctypes.data, lr_shift, mode, desc_of(net), w.ctypes.data, err.ctypes.data,
                                               mag.ctypes.data, tr.depth, tr.lam, hist.ctypes.data, ln.ctypes.data, tr.slot) == 0
    return w.astype(np.int64), err, mag


def want_tables(net, tc=None):
    """(weights,) or (weights, err, mag): compact, flat int64 of a reference network and its accumulators, as host_update and
    the GPU tests' ``tables`` give them."""
    w = mref.flat_of(net).reshape(-1)
    if tc is None:
        return (w,)
    err, mag = mref.tc_flat(tc, net)
    return w, err.reshape(-1), mag.reshape(-1)


# ------------------------------------------------------------------------------------------------ shared reference results
THR_3 = (sref.stage_mask(4), sref.stage_mask(16, 8))    # S = 3 on small boards: a spawned 4 alone crosses the first


def net_of(name, thr=()):
    """The reference network of shape ``name`` (ntuple_mixed_ref.SHAPES): full-range random int32 over the whole compact array,
    a different table per stage."""
    tuples = mref.SHAPES[name]
    return cached(("net", name, thr), lambda: mref.mixed_net(tuples, thr, 10, mref.random_flat(tuples, 91, len(thr) + 1)))


def shallow(name):
    """The reference on boards_67 under net_of(name), computed once: (values, evaluate, search depth 1)."""
    return cached(("shallow", name), lambda: (sref.values_batch(boards_67(), net_of(name)), sref.evaluate_batch(boards_67(), net_of(name)),
                                              sref.search_batch(boards_67(), 1, net_of(name))))


def deep(name):
    """Search depth 2 of the reference on near_full_12, computed once."""
    return cached(("deep", name), lambda: sref.search_batch(near_full_12(), 2, net_of(name), {"memo": {}}))


def staged_boards():
    """61 small boards, which the low thresholds THR_3 put into every stage, and the three edge boards."""
    return cached("staged boards", lambda: np.concatenate([small_boards(61, 92), mref.edge_boards()]))


def random_tc(net, seed):
    """Reference accumulators that are random over the whole compact array (ntuple_tc_helpers.preload's distribution)."""
    S, W = net.n_stages, mref.n_weights(net.tuples)
    flat = preload(types.SimpleNamespace(weights=np.empty((S, W))), seed)
    return mref.tc_of(net, flat.err, flat.mag_i64())


def pushed_trace(n, H, lam, seed):
    """A reference trace after H + 2 synthetic pushes whose newest slot holds the edge boards for boards 0..2."""
    tr = tref.Trace(n, H, lam)
    for after, av, best, term in push_inputs(n, H + 2, seed):
        tref.push(tr, after, av, best, term)
    tr.hist[tr.slot, :3] = mref.edge_boards()
    tr.len[:3] = 1
    return tr
