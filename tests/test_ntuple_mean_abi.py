"""CPU: the batch-mean n-tuple update (g2048_ntuple_mean_update_plain, g2048_ntuple_mean_trace_update and their staged siblings,
INTEGRATION.md §22) at the library's and the Python layer's doors, without a GPU: the four symbols are exported and bound, the
struct has the header's layout, the ABI number has not moved, every argument the definition rules out is refused before any HIP
call (the addresses below are fake: a call that got past its checks would fault), and the Python wrappers raise their ValueErrors
before any launch.  The first test fails on the parent commit: the symbols do not exist there."""
import ctypes as C
import inspect

import pytest

import __graft_entry__ as ge
from ntuple_helpers import TUPLES_17x4

BUF, OUT, WEIGHTS, SUM, COUNT = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000     # fake device addresses
PLAIN = ("g2048_ntuple_mean_update_plain", "g2048_ntuple_staged_mean_update_plain")
TRACE = ("g2048_ntuple_mean_trace_update", "g2048_ntuple_staged_mean_trace_update")


@pytest.fixture(scope="module")
def lib():
    ge.build_hip()
    from gym2048_amd import _lib
    return _lib.load()


def _net(staged):
    from gym2048_amd import _lib
    net = _lib.NTupleNetC(5, 4, 10)
    for t, cells in enumerate(TUPLES_17x4):
        for k, c in enumerate(cells):
            net.cells[t][k] = c
    net.weights = WEIGHTS
    return _lib.NTupleStagedNetC(net, 1) if staged else net


def _mean(sum=SUM, count=COUNT):
    from gym2048_amd import _lib
    return _lib.NTupleMeanC(sum, count)


def _trace(depth=4):
    from gym2048_amd import _lib
    return _lib.NTupleTraceC(depth, 32768, BUF, BUF)


def refused(lib, rc, *words):
    msg = lib.g2048_last_error()
    assert rc == -1 and msg and all(w in msg for w in words), (rc, msg)


def test_symbols_are_exported_and_bound_and_the_abi_is_still_16(lib):
    from gym2048_amd import _lib
    mean_p, tr_p, u32, u64, P = C.POINTER(_lib.NTupleMeanC), C.POINTER(_lib.NTupleTraceC), C.c_uint32, C.c_uint64, C.c_void_p
    net_p, staged_p = C.POINTER(_lib.NTupleNetC), C.POINTER(_lib.NTupleStagedNetC)
    want = {"g2048_ntuple_mean_update_plain": [P, u64, P, u32, u32, net_p, mean_p, P],
            "g2048_ntuple_staged_mean_update_plain": [P, u64, P, u32, u32, staged_p, mean_p, P],
            "g2048_ntuple_mean_trace_update": [u64, P, u32, u32, net_p, mean_p, tr_p, u32, P],
            "g2048_ntuple_staged_mean_trace_update": [u64, P, u32, u32, staged_p, mean_p, tr_p, u32, P]}
    for name, argtypes in want.items():
        assert hasattr(lib, name)
        assert _lib.SIGNATURES[name] == (C.c_int, argtypes)
    assert lib.g2048_abi_version() == _lib.ABI_VERSION == 16
    assert [f[0] for f in _lib.NTupleMeanC._fields_] == ["sum", "count"] and C.sizeof(_lib.NTupleMeanC) == 16
    # the order of the TC forms, with the state where they have the accumulators
    for name in want:
        tc = _lib.SIGNATURES[name.replace("mean", "tc")][1]
        assert [a if a is not C.POINTER(_lib.NTupleTCC) else mean_p for a in tc] == want[name]


def calls(lib):
    """(name, staged, call(net, mean, n=64, lr_shift=4, phases=3, depth=4)) of the four entry points."""
    out = []
    for name in PLAIN:
        out.append((name, "staged" in name, lambda net, mean, n=64, lr_shift=4, phases=3, depth=4, fn=getattr(lib, name):
                    fn(BUF, n, OUT, lr_shift, phases, net, mean, None)))
    for name in TRACE:
        out.append((name, "staged" in name, lambda net, mean, n=64, lr_shift=4, phases=3, depth=4, fn=getattr(lib, name):
                    fn(n, OUT, lr_shift, phases, net, mean, C.byref(_trace(depth)), depth - 1, None)))
    return out


def test_refusals_without_a_device(lib):
    for name, staged, call in calls(lib):
        net = C.byref(_net(staged))
        for phases in (0, 4, 7):
            refused(lib, call(net, C.byref(_mean()), phases=phases), b"phases=%d" % phases)
        refused(lib, call(net, C.byref(_mean()), lr_shift=41), b"lr_shift=41")
        refused(lib, call(net, None), b"mean is NULL")
        refused(lib, call(net, C.byref(_mean(sum=None))), b"mean sum is NULL")
        refused(lib, call(net, C.byref(_mean(count=None))), b"mean count is NULL")
        refused(lib, call(net, C.byref(_mean(sum=SUM + 4))), b"misaligned", b"sum needs 8 bytes")
        for off in (1, 2, 3):
            refused(lib, call(net, C.byref(_mean(count=COUNT + off))), b"misaligned", b"count needs 4 bytes")
        # the checks of the TC forms
        refused(lib, call(None, C.byref(_mean())), b"net is NULL")
        refused(lib, call(net, C.byref(_mean()), n=0), b"n=0")
        bad = _net(staged)
        (bad.net if staged else bad).n_tuples = 9
        refused(lib, call(C.byref(bad), C.byref(_mean())), b"n_tuples=9")


def test_the_item_bound(lib):
    """H * n >= 2^29 is refused, H * n = 2^29 - 1 (or the nearest below) is not refused for its size: phases = 0 is what is
    refused then, so no launch happens here."""
    for name, staged, call in calls(lib):
        net, mean = C.byref(_net(staged)), C.byref(_mean())
        if "trace" in name:
            for depth, n in ((4, 1 << 27), (8, 1 << 26), (1, 1 << 29), (3, (1 << 29) // 3 + 1)):
                assert depth * n >= 1 << 29
                refused(lib, call(net, mean, n=n, depth=depth), b"2^29")
            for depth, n in ((4, (1 << 27) - 1), (1, (1 << 29) - 1), (3, (1 << 29) // 3)):
                assert depth * n < 1 << 29
                refused(lib, call(net, mean, n=n, depth=depth, phases=0), b"phases=0")
        else:
            refused(lib, call(net, mean, n=1 << 29), b"2^29")
            refused(lib, call(net, mean, n=(1 << 32) - 256), b"2^29")
            refused(lib, call(net, mean, n=(1 << 29) - 1, phases=0), b"phases=0")


# ------------------------------------------------------------------------------------------------ the Python layer
def test_python_wrappers_check_their_arguments_before_the_library():
    import torch
    from gym2048_amd import ntuple
    net, other = ntuple.NTupleNet("17x4", device="cpu"), ntuple.NTupleNet("17x4", device="cpu")
    mean = ntuple.NTupleMean(net)
    assert mean.sum.dtype == torch.int64 and mean.count.dtype == torch.int32 and mean.sum.shape == mean.count.shape == net.weights.shape
    small = ntuple.NTupleNet(((0, 1), (5,)), device="cpu", stages=(ntuple.stage_mask(8),), mixed=True)
    assert ntuple.NTupleMean(small).sum.shape == ntuple.NTupleMean(small).count.shape == small.weights.shape == (2, 272)
    mean.sum += 3
    mean.count += 1
    mean.reset()
    assert not mean.sum.any() and not mean.count.any()
    with pytest.raises(ValueError, match="net must be an NTupleNet"):
        ntuple.NTupleMean(object())
    boards, delta = torch.zeros((8, 16), dtype=torch.uint8), torch.zeros(8, dtype=torch.int64)
    trace = ntuple.NTupleTrace(8, depth=2, device="cpu")
    with pytest.raises(ValueError, match="boards must be"):              # (plain boards are checked first, and must be on a GPU)
        net.mean_update(boards, delta, 4, mean)
    for call in (lambda **kw: net.mean_trace_update(**{"trace": trace, "delta": delta, "lr_shift": 4, "mean": mean, **kw}),):
        with pytest.raises(ValueError, match="mean must be the NTupleMean of this network"):
            call(mean=ntuple.NTupleMean(other))
        with pytest.raises(ValueError, match="mean must be the NTupleMean of this network"):
            call(mean=ntuple.NTupleTC(net))
        for phases in (0, 4, 1.0):
            with pytest.raises(ValueError, match="phases"):
                call(phases=phases)
        for shift in (-1, 41):
            with pytest.raises(ValueError, match="lr_shift"):
                call(lr_shift=shift)
        with pytest.raises(ValueError, match="delta must be a contiguous int64"):
            call(delta=torch.zeros(8, dtype=torch.int32))
    with pytest.raises(ValueError, match="trace must be an NTupleTrace"):
        net.mean_trace_update(object(), delta, 4, mean)


def test_trainers_have_the_signatures_of_the_tc_family():
    import gym2048_amd
    from gym2048_amd import ntuple
    for name, twin in (("mean_update", "tc_update"), ("mean_step", "tc_step"), ("mean_train", "tc_train"), ("mean_tdl_step", "tcl_step"),
                       ("mean_tdl_train", "tcl_train")):
        mine, theirs = list(inspect.signature(getattr(ntuple, name)).parameters), list(inspect.signature(getattr(ntuple, twin)).parameters)
        assert mine == ["mean" if p == "tc" else p for p in theirs], name
        assert getattr(gym2048_amd, name) is getattr(ntuple, name)
    assert gym2048_amd.NTupleMean is ntuple.NTupleMean
    for name in ("mean_step", "mean_train", "mean_tdl_step", "mean_tdl_train"):
        params = inspect.signature(getattr(ntuple, name)).parameters
        assert params["fused"].default is False and params["carousel"].default is None
    with pytest.raises(ValueError, match="fused=True cannot run a carousel"):
        net = ntuple.NTupleNet("17x4", device="cpu")
        ntuple.mean_train(None, net, ntuple.NTupleMean(net), 2, 4, carousel=object(), fused=True)
