"""Shared by the batch-mean n-tuple tests: the host build of the header's two per-item operations (tests/host_ntuple_mean, g++)
behind ctypes, the comparison of the three tables, a vectorised numpy form of the reference for batches of thousands of boards,
and the device's side of a reference network.  A plain module, like ntuple_mixed_helpers."""
import ctypes as C

import numpy as np

import host_build
import ntuple_mean_ref as meanref
import ntuple_mixed_ref as mref
import ntuple_staged_ref as sref
import ntuple_tc_ref as tcref
import ntuple_trace_ref as tref
from host_build import Desc
from ntuple_tc_helpers import assert_tables_equal

NAMES = ("weights", "sum", "count")
KIND = {"uniform": 0, "staged": 1, "mixed": 2}


def desc_of(net, kind=2):
    """The description of a reference network (ntuple_mixed_ref.mixed_net): END-padded lists up to the longest one.  kind 0 / 1
    (NtupleShape / NtupleStagedShape) are for lists of one length only: there [S][T][16^L] is the compact layout."""
    assert kind == 2 or len(set(mref.lens(net.tuples))) == 1
    return host_build.desc_of(net, kind)


def build_host_mean(force=False):
    return host_build.build_host("host_ntuple_mean", "mean_check.cpp", "libmean_check.so", force)


def load_host_mean():
    lib = C.CDLL(build_host_mean())
    P, u32, u64, D = C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(Desc)
    for name, argtypes in (("floor_div", [C.c_int64, u32, P]), ("update", [P, u64, P, u32, u32, D, P, P, P, P, u64]),
                           ("trace_update", [u64, P, u32, u32, D, P, P, P, u32, u32, P, P, u32, P, u64])):
        f = getattr(lib, "mean_check_" + name)
        f.restype, f.argtypes = C.c_int, argtypes
    return lib


# ------------------------------------------------------------------------------------------------ tables
def want_tables(net, mean):
    """(weights, sum, count): compact, flat int64 of a reference network and its mean state."""
    return tuple(mref.compact(a, net.tuples).astype(np.int64).reshape(-1) for a in (net.weights, mean.sum, mean.count))


def mean_of(net, flat_sum=None, flat_count=None):
    """A reference Mean of ``net`` from compact [S, W] arrays, zero when None."""
    mean = meanref.Mean(net)
    if flat_sum is not None:
        S = net.n_stages
        mean.sum[:] = mref.expand(np.asarray(flat_sum).reshape(S, -1), net.tuples)
        mean.count[:] = mref.expand(np.asarray(flat_count).reshape(S, -1), net.tuples).astype(np.uint32)
    return mean


def _host_tables(net, mean):
    w = np.ascontiguousarray(mref.flat_of(net).astype(np.int32).reshape(-1))
    s = np.ascontiguousarray(mref.compact(mean.sum, net.tuples).reshape(-1))
    c = np.ascontiguousarray(mref.compact(mean.count, net.tuples).astype(np.uint32).reshape(-1))
    return w, s, c


def _order(order):
    if order is None:
        return None, 0
    o = np.ascontiguousarray(np.asarray(order, np.uint64))
    return o, len(o)


def host_update(lib, boards, deltas, lr_shift, phases, net, mean, order=None, kind=2):
    """(weights, sum, count) as compact flat int64 after the host build's update (``net`` and ``mean`` are not modified);
    ``order``: a permutation of the board numbers."""
    b = np.ascontiguousarray(np.asarray(boards, np.uint8).reshape(-1, 16))
    d = np.ascontiguousarray(np.asarray(deltas, np.int64))
    w, s, c = _host_tables(net, mean)
    o, n_o = _order(order)
    assert lib.mean_check_update(b.ctypes.data, len(b), d.ctypes.data, lr_shift, phases, desc_of(net, kind), w.ctypes.data, s.ctypes.data,
                                 c.ctypes.data, None if o is None else o.ctypes.data, n_o) == 0
    return w.astype(np.int64), s, c.astype(np.int64)


def host_trace_update(lib, tr, deltas, lr_shift, phases, net, mean, order=None, kind=2):
    """The same for the trace items; ``order``: a permutation of the H * n item numbers k * n + i."""
    d = np.ascontiguousarray(np.asarray(deltas, np.int64))
    w, s, c = _host_tables(net, mean)
    hist, ln = np.ascontiguousarray(tr.hist), np.ascontiguousarray(tr.len)
    o, n_o = _order(order)
    assert lib.mean_check_trace_update(tr.n, d.ctypes.data, lr_shift, phases, desc_of(net, kind), w.ctypes.data, s.ctypes.data, c.ctypes.data,
                                       tr.depth, tr.lam, hist.ctypes.data, ln.ctypes.data, tr.slot,
                                       None if o is None else o.ctypes.data, n_o) == 0
    return w.astype(np.int64), s, c.astype(np.int64)


def orders(n, seed=5):
    """Forward (the header's own loop), reverse and a shuffled order of n items."""
    return None, np.arange(n)[::-1], np.random.default_rng(seed).permutation(n)


def assert_mean_tables(got, want, where=""):
    assert_tables_equal(got, want, names=tuple(f"{where}{x}" for x in NAMES))


# ------------------------------------------------------------------------------------------------ the update matrix
def matrix_case(family, T, source):
    """The batch-mean update of an ntuple_update_matrix case (its networks, boards, ring and deltas; zero state), computed once:
    ``case`` (the matrix's own), ``want`` (the Expected weights), ``trace`` of the reference."""
    import types

    import ntuple_update_matrix as um

    def make():
        net, _ = um.family_net(family, T)
        mean, trace = meanref.Mean(net), {}
        case = um.case_of(family, T, source)
        if source == "board":
            meanref.mean_update(net, mean, case.boards, case.deltas, case.lr_shift, 3, trace)
        else:
            meanref.mean_trace_update(net, mean, case.tr, case.deltas, case.lr_shift, 3, trace)
        assert mean.is_zero()
        return types.SimpleNamespace(case=case, want=um.Expected(um.base_tables(family, T)[:1], want_tables(net, mean)[:1]), trace=trace)
    return um.cached(("mean", family, T, source), make)


def assert_matrix_conditions(family, T, source):
    """What the references and the inputs say about a matrix case -- nothing here has seen the code under test."""
    import ntuple_update_matrix as um
    c, tuples, S = matrix_case(family, T, source), um.family_tuples(family, T), len(um.family_thr(family)) + 1
    base = um.base_tables(family, T)[:1]
    # every table of every stage is written: the instantiation of T - 1 leaves table T - 1 as it was, the uniform shape every
    # stage but the first
    assert um.tables_hit(c.want.idx[0], tuples, S) == um.every_table(tuples, S), "inputs: the weights do not change in every table of every stage"
    # every table has an entry that is not a plain update's: reached at least twice
    assert set(c.trace["by_table"]) == um.every_table(tuples, S) and min(c.trace["by_table"].values()) >= 2, "inputs: a table without a count >= 2"
    assert c.trace["multi"] > 0 and c.trace["sym"] > 0, "inputs: entries reached by two items, and twice by one"
    assert source != "board" or c.trace["zero"] > 0, "inputs: items with d == 0"
    # an entry point that reached the summed update's kernel would give its weights
    assert (c.want.on(base)[0] != c.case.td.on(base)[0]).any(), "inputs: the mean weights are the TD weights"
    if T > 1:
        Wn, Wp = mref.n_weights(tuples), mref.n_weights(tuples[:-1])
        prev = matrix_case(family, T - 1, source).want.on(um.base_tables(family, T - 1)[:1])[0]
        left = base[0].copy().reshape(S, Wn)
        left[:, :Wp] = prev.reshape(S, Wp)
        assert (left.reshape(-1) != c.want.on(base)[0]).any(), "inputs: the neighbouring instantiation would leave the same tables"


# ------------------------------------------------------------------------------------------------ whole arrays
def mean_steps_np(tuples, boards, deltas, lr_shift, thr=()):
    """(elements, steps, counts): the distinct compact elements (stage * W + base_t + idx) a batch reaches, the step each takes
    and its count, with numpy arithmetic on whole arrays -- for thousands of boards.  |delta| <= 2^40 after the clamp and fewer
    than 2^19 items: the int64 sums cannot wrap.  tests/test_ntuple_mean_host.py pins it to the scalar reference."""
    boards = np.asarray(boards, np.uint8).reshape(-1, 16)
    d = np.clip(np.asarray(deltas, np.int64), -tcref.MAX_DELTA, tcref.MAX_DELTA)
    assert len(boards) == len(d) < 1 << 19
    live = np.nonzero(d)[0]
    if len(live) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    W, bases = mref.n_weights(tuples), mref.bases(tuples)
    net = sref._view([tuple(t) for t in tuples], 0, None)
    idx = tref.offsets_np(boards[live], net)                                         # [8, T, m]
    stage = sref.stage_batch(boards[live], thr).astype(np.int64) if thr else np.zeros(len(live), np.int64)
    elem = idx + np.array(bases, np.int64)[None, :, None] + (stage * W)[None, None, :]
    elem, dd = elem.reshape(-1), np.broadcast_to(d[live], idx.shape).reshape(-1)
    uniq, inv = np.unique(elem, return_inverse=True)
    total, count = np.zeros(len(uniq), np.int64), np.zeros(len(uniq), np.int64)
    np.add.at(total, inv, dd)
    np.add.at(count, inv, 1)
    step = np.clip((total // count) >> lr_shift, -(1 << 31), (1 << 31) - 1)          # numpy's // and >> on int64 floor
    return uniq, step, count


def wrap32_np(x):
    return (x + (1 << 31)) % (1 << 32) - (1 << 31)


def mean_update_np(weights, tuples, boards, deltas, lr_shift, thr=()):
    """The batch-mean update of ``weights`` (compact flat int64 [S * W] holding int32 values), in place, by mean_steps_np."""
    elem, step, _ = mean_steps_np(tuples, boards, deltas, lr_shift, thr)
    weights[elem] = wrap32_np(weights[elem] + step)
    return weights


def trace_items_np(tr, deltas):
    """(boards, d_k) of every trace item with k < L, k-major, as whole arrays (d_k may be 0: mean_update_np drops those)."""
    H = tr.depth
    d = np.clip(np.asarray(deltas, np.int64), -tcref.MAX_DELTA, tcref.MAX_DELTA)
    L = np.minimum(tr.len & 0x7f, H)
    boards, dks = [], []
    for k in range(H):
        live = np.nonzero(k < L)[0]
        boards.append(tr.hist[(tr.slot + H - k) % H][live])
        dks.append((d[live] * tref.decay(tr.lam, k)) >> 16)
    return np.concatenate(boards), np.concatenate(dks)


# ------------------------------------------------------------------------------------------------ the device
def device_state(g, torch, rnet, rmean=None):
    """(NTupleNet, NTupleMean) on the GPU with the lists, stages and weights of a reference network; the state is zero, or
    ``rmean``'s."""
    net = g.NTupleNet(rnet.tuples, frac_bits=rnet.frac_bits, stages=rnet.thr or None, mixed=True)
    net.weights.copy_(torch.as_tensor(mref.flat_of(rnet).astype(np.int32)).reshape(net.weights.shape))
    mean = g.NTupleMean(net)
    if rmean is not None:
        _, s, c = _host_tables(rnet, rmean)
        mean.sum.copy_(torch.as_tensor(s).reshape(mean.sum.shape))
        mean.count.copy_(torch.as_tensor(c.view(np.int32)).reshape(mean.count.shape))
    return net, mean


def tables(net, mean):
    """The device's arrays as flat int64, as want_tables gives the reference's (count read as unsigned)."""
    return (net.weights.cpu().numpy().astype(np.int64).reshape(-1), mean.sum.cpu().numpy().reshape(-1),
            mean.count.cpu().numpy().view(np.uint32).astype(np.int64).reshape(-1))
