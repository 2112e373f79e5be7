"""CPU: the n-tuple move log and backward learning (g2048_ntuple_play_log, g2048_ntuple_log_delta, g2048_ntuple_log_sweep,
g2048_ntuple_log_train and their staged siblings) at the library's and the Python layer's doors, without a
GPU: the eight symbols are exported and bound, the struct has the header's layout, the ABI number has not moved, everything the
library can refuse without an engine or a device it refuses before it looks at either (a NULL engine shows every such refusal
of the engine forms, with its message; the plain forms are refused before any HIP call; the one refusal that needs a live
engine, numpy-RNG mode, is in test_gpu_ntuple_log.py), and the Python wrappers raise their ValueErrors before any launch.  The
first test fails on the parent commit: the symbols do not exist there."""
import ctypes as C
import types

import pytest

import __graft_entry__ as ge
from ntuple_helpers import TUPLES_17x4

WEIGHTS, AFTER, GAIN, FLAG, DELTA, ACC = 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000   # fake device addresses: never used
N = 64
FORMS = ("", "staged_")


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


def _log(**kw):
    from gym2048_amd import _lib
    log = _lib.NTupleLogC(4, AFTER, GAIN, FLAG)
    for name, v in kw.items():
        setattr(log, name, v)
    return log


def refused(lib, rc, *words):
    msg = lib.g2048_last_error()
    assert rc == -1 and msg and all(w in msg for w in words), (rc, msg)


def test_symbols_are_exported_and_bound_and_the_abi_is_still_16(lib):
    from gym2048_amd import _lib
    log_p, tc_p, u32, u64, P = C.POINTER(_lib.NTupleLogC), C.POINTER(_lib.NTupleTCC), C.c_uint32, C.c_uint64, C.c_void_p
    for prefix, net_p in (("g2048_ntuple_", C.POINTER(_lib.NTupleNetC)), ("g2048_ntuple_staged_", C.POINTER(_lib.NTupleStagedNetC))):
        want = {prefix + "play_log": [P, net_p, log_p, P],
                prefix + "log_delta": [u64, net_p, log_p, u32, P, P],
                prefix + "log_sweep": [u64, net_p, log_p, u32, P, tc_p, P],
                prefix + "log_train": [P, net_p, u32, u32, log_p, P, tc_p, P]}
        for name, argtypes in want.items():
            assert hasattr(lib, name)
            assert _lib.SIGNATURES[name] == (C.c_int, argtypes)
    assert lib.g2048_abi_version() == _lib.ABI_VERSION == 16
    assert [f[0] for f in _lib.NTupleLogC._fields_] == ["depth", "after", "gain", "flag"]
    assert C.sizeof(_lib.NTupleLogC) == 32
    from gym2048_amd import ntuple
    assert (ntuple.LOG_MAX_DEPTH, ntuple.LOG_VALID, ntuple.LOG_ENDED) == (1024, 1, 2)
    header = open(ge.os.path.join(ge.ROOT, "include", "g2048.h")).read()
    for line in ("#define G2048_NTUPLE_LOG_MAX_DEPTH 1024", "#define G2048_NTUPLE_LOG_VALID 1u", "#define G2048_NTUPLE_LOG_ENDED 2u"):
        assert line in header


def calls(lib):
    """(name, staged, call(net, log)) of the eight entry points with everything else in order: the engine forms with a NULL
    engine, the trainers at rounds 3, lr_shift 4, TD; log_delta at m = 0."""
    out = []
    for form in FORMS:
        staged = bool(form)
        fn = lambda name: getattr(lib, "g2048_ntuple_" + form + name)   # noqa: E731
        out.append(("play_log", staged, lambda net, log, f=fn("play_log"): f(None, net, log, None)))
        out.append(("log_delta", staged, lambda net, log, f=fn("log_delta"): f(N, net, log, 0, DELTA, None)))
        out.append(("log_sweep", staged, lambda net, log, f=fn("log_sweep"): f(N, net, log, 4, DELTA, None, None)))
        out.append(("log_train", staged, lambda net, log, f=fn("log_train"): f(None, net, 3, 4, log, DELTA, None, None)))
    return out


def test_refusals_without_a_device(lib):
    for name, staged, call in calls(lib):
        net = _net(staged)
        if name in ("play_log", "log_train"):                            # everything in order but the engine
            refused(lib, call(C.byref(net), C.byref(_log())), b"engine is NULL")
        refused(lib, call(None, C.byref(_log())), b"net is NULL")
        refused(lib, call(C.byref(net), None), b"log is NULL")
        # a descriptor g2048_ntuple_play refuses
        for field, value, word in (("n_tuples", 0, b"n_tuples=0"), ("n_tuples", 9, b"n_tuples=9"), ("tuple_len", 7, b"tuple_len=7"),
                                   ("frac_bits", 17, b"frac_bits=17"), ("weights", None, b"weights is NULL"),
                                   ("weights", WEIGHTS + 8, b"misaligned")):
            bad = _net(staged)
            setattr(bad.net if staged else bad, field, value)
            refused(lib, call(C.byref(bad), C.byref(_log())), word)
        if staged:
            bad = _net(True)
            bad.n_stages = 9
            refused(lib, call(C.byref(bad), C.byref(_log())), b"n_stages=9")
        # the log: a NULL member, a depth outside 1..1024, a misaligned pointer
        for member in ("after", "gain", "flag"):
            refused(lib, call(C.byref(net), C.byref(_log(**{member: None}))), b"log " + member.encode() + b" is NULL")
        for depth in (0, 1025, 0xffffffff):
            refused(lib, call(C.byref(net), C.byref(_log(depth=depth))), b"depth=%d" % depth, b"1 <= depth <= 1024")
        refused(lib, call(C.byref(net), C.byref(_log(after=AFTER + 8))), b"misaligned", b"log after needs 16 bytes")
        refused(lib, call(C.byref(net), C.byref(_log(gain=GAIN + 4))), b"misaligned", b"log gain needs 8 bytes")
        # in either order of discovery: a bad log with a bad net, a bad log with a NULL engine
        refused(lib, call(None, None), b"is NULL")
        bad = _net(staged)
        (bad.net if staged else bad).n_tuples = 9
        refused(lib, call(C.byref(bad), C.byref(_log(depth=0))), b"=")
    for form in FORMS:                                                   # bytes: any address; depth 1 and 1024 are in range
        net = _net(bool(form))
        fn = getattr(lib, "g2048_ntuple_" + form + "play_log")
        refused(lib, fn(None, C.byref(net), C.byref(_log(flag=FLAG + 1)), None), b"engine is NULL")
        for depth in (1, 1024):
            refused(lib, fn(None, C.byref(net), C.byref(_log(depth=depth)), None), b"engine is NULL")


def test_log_delta_refusals_without_a_device(lib):
    for form in FORMS:
        net = _net(bool(form))
        fn = getattr(lib, "g2048_ntuple_" + form + "log_delta")
        for m in (4, 5, 0xffffffff):                                     # depth 4: slots 0..3 have a successor
            refused(lib, fn(N, C.byref(net), C.byref(_log()), m, DELTA, None), b"m=%d" % m, b"depth=4")
        refused(lib, fn(N, C.byref(net), C.byref(_log()), 0, None, None), b"delta is NULL")
        refused(lib, fn(N, C.byref(net), C.byref(_log()), 0, DELTA + 4, None), b"misaligned", b"delta")
        refused(lib, fn(0, C.byref(net), C.byref(_log()), 0, DELTA, None), b"n=0")
        refused(lib, fn(1 << 32, C.byref(net), C.byref(_log()), 0, DELTA, None), b"n=4294967296")


def test_sweep_and_train_refusals_without_a_device(lib):
    from gym2048_amd import _lib
    for form in FORMS:
        net = _net(bool(form))
        sweep = lambda lr=4, delta=DELTA, tc=None, f=getattr(lib, "g2048_ntuple_" + form + "log_sweep"): \
            f(N, C.byref(net), C.byref(_log()), lr, delta, tc, None)    # noqa: E731
        train = lambda lr=4, delta=DELTA, tc=None, rounds=3, f=getattr(lib, "g2048_ntuple_" + form + "log_train"): \
            f(None, C.byref(net), rounds, lr, C.byref(_log()), delta, tc, None)   # noqa: E731
        for call in (sweep, train):
            refused(lib, call(lr=41), b"lr_shift=41")
            refused(lib, call(delta=None), b"delta is NULL")
            refused(lib, call(delta=DELTA + 4), b"misaligned", b"delta")
            # a tc g2048_ntuple_tc_update_plain refuses
            refused(lib, call(tc=C.byref(_lib.NTupleTCC(None, ACC))), b"tc err is NULL")
            refused(lib, call(tc=C.byref(_lib.NTupleTCC(ACC, None))), b"tc mag is NULL")
            refused(lib, call(tc=C.byref(_lib.NTupleTCC(ACC + 4, ACC))), b"misaligned", b"tc")
        refused(lib, train(lr=40), b"engine is NULL")
        refused(lib, train(tc=C.byref(_lib.NTupleTCC(ACC, ACC))), b"engine is NULL")
        # rounds == 0 does not excuse a bad argument, and the engine is still looked at
        refused(lib, train(lr=41, rounds=0), b"lr_shift=41")
        refused(lib, train(rounds=0), b"engine is NULL")
        fn = getattr(lib, "g2048_ntuple_" + form + "log_sweep")
        refused(lib, fn(0, C.byref(net), C.byref(_log()), 4, DELTA, None, None), b"n=0")


# ------------------------------------------------------------------------------------------------ the Python layer
def _engine(torch, n=8):
    """A Batched2048 that has no device behind it: enough for the checks that come before the library call."""
    from gym2048_amd.batched import Batched2048
    eng = Batched2048.__new__(Batched2048)
    eng._h, eng.n_envs, eng.device = None, n, torch.device("cpu")
    eng._lib = types.SimpleNamespace(g2048_destroy=lambda h: 0)
    eng.terminated = torch.zeros(n, dtype=torch.uint8)
    return eng


def test_the_log_object():
    import torch
    from gym2048_amd import ntuple
    log = ntuple.NTupleLog(8, depth=3, device="cpu")
    assert (log.n, log.depth) == (8, 3) and ntuple.NTupleLog(8, device="cpu").depth == 16
    assert log.after.shape == (4, 8, 16) and log.after.dtype == torch.uint8
    assert log.gain.shape == (4, 8) and log.gain.dtype == torch.int64
    assert log.flag.shape == (4, 8) and log.flag.dtype == torch.uint8
    assert not log.after.any() and not log.gain.any() and not log.flag.any()
    assert (log._c.depth, log._c.after, log._c.gain, log._c.flag) == (3, log.after.data_ptr(), log.gain.data_ptr(), log.flag.data_ptr())
    assert log.slot(2).shape == (8, 16) and log.slot(2).data_ptr() == log.after[2].data_ptr() and log.slot(3).is_contiguous()
    for bad in (-1, 4, 1.5):
        with pytest.raises(ValueError, match="m"):
            log.slot(bad)
    for kw in (dict(depth=0), dict(depth=1025), dict(depth=2.5), dict(n=0)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            ntuple.NTupleLog(**{"n": 8, "device": "cpu", **kw})
    log.after.fill_(3), log.gain.fill_(-5), log.flag.fill_(1)
    state = log.state_dict()
    other = ntuple.NTupleLog(8, depth=3, device="cpu")
    other.load_state_dict(state)
    assert torch.equal(other.after, log.after) and torch.equal(other.gain, log.gain) and torch.equal(other.flag, log.flag)
    assert state["after"].data_ptr() != log.after.data_ptr()
    with pytest.raises(ValueError, match="depth"):
        ntuple.NTupleLog(8, depth=2, device="cpu").load_state_dict(state)
    with pytest.raises(ValueError, match="state_dict gain must be int64"):
        other.load_state_dict({**state, "gain": state["gain"].to(torch.int32)})
    with pytest.raises(ValueError, match=r"state_dict after must be uint8 \(4, 9, 16\)"):
        ntuple.NTupleLog(9, depth=3, device="cpu").load_state_dict(state)
    log.reset()
    assert not log.after.any() and not log.gain.any() and not log.flag.any()


def test_python_wrappers_check_their_arguments_before_the_library():
    import torch
    import gym2048_amd
    from gym2048_amd import ntuple
    assert gym2048_amd.NTupleLog is ntuple.NTupleLog and gym2048_amd.log_sweep is ntuple.log_sweep
    assert gym2048_amd.backward_train is ntuple.backward_train
    eng, net = _engine(torch), ntuple.NTupleNet("17x4", device="cpu")
    log, delta = ntuple.NTupleLog(8, depth=2, device="cpu"), torch.zeros(8, dtype=torch.int64)
    other = ntuple.NTupleNet("17x4", device="cpu")
    # the engine's methods
    for call in (lambda **kw: eng.ntuple_play_log(**{"net": net, "log": log, **kw}),
                 lambda **kw: eng.ntuple_log_train(**{"net": net, "log": log, "rounds": 1, "lr_shift": 4, "delta": delta, **kw})):
        with pytest.raises(ValueError, match="net must be an NTupleNet"):
            call(net=object())
        with pytest.raises(ValueError, match="log must be an NTupleLog of 8 boards"):
            call(log=object())
        with pytest.raises(ValueError, match="log must be an NTupleLog of 8 boards"):
            call(log=ntuple.NTupleLog(9, depth=2, device="cpu"))
    for kw in (dict(rounds=-1), dict(rounds=1 << 32), dict(rounds=1.5), dict(lr_shift=41), dict(lr_shift=-1)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            eng.ntuple_log_train(**{"net": net, "log": log, "rounds": 1, "lr_shift": 4, "delta": delta, **kw})
    with pytest.raises(ValueError, match="delta must be a contiguous int64"):
        eng.ntuple_log_train(net, log, 1, 4, torch.zeros(8, dtype=torch.int32))
    with pytest.raises(ValueError, match="tc must be the NTupleTC of this network"):
        eng.ntuple_log_train(net, log, 1, 4, delta, tc=ntuple.NTupleTC(other))
    # NTupleNet.log_delta
    with pytest.raises(ValueError, match="log must be an NTupleLog"):
        net.log_delta(object(), 0)
    for m in (-1, 2, 0.5):
        with pytest.raises(ValueError, match="m"):
            net.log_delta(log, m)
    with pytest.raises(ValueError, match="out must be a contiguous int64"):
        net.log_delta(log, 0, out=torch.zeros(9, dtype=torch.int64))
    # log_sweep and backward_train
    with pytest.raises(ValueError, match="net must be an NTupleNet"):
        ntuple.log_sweep(object(), log, 4)
    with pytest.raises(ValueError, match="log must be an NTupleLog"):
        ntuple.log_sweep(net, object(), 4)
    with pytest.raises(ValueError, match="lr_shift"):
        ntuple.log_sweep(net, log, 41)
    with pytest.raises(ValueError, match="tc must be the NTupleTC of this network"):
        ntuple.log_sweep(net, log, 4, tc=ntuple.NTupleTC(other))
    with pytest.raises(ValueError, match="mean must be the NTupleMean of this network"):
        ntuple.log_sweep(net, log, 4, mean=ntuple.NTupleMean(other))
    with pytest.raises(ValueError, match="tc or mean, not both"):
        ntuple.log_sweep(net, log, 4, tc=ntuple.NTupleTC(net), mean=ntuple.NTupleMean(net))
    with pytest.raises(ValueError, match="delta must be a contiguous int64"):
        ntuple.log_sweep(net, log, 4, delta=torch.zeros((8, 1), dtype=torch.int64))
    with pytest.raises(ValueError, match="backward_train cannot run a carousel"):
        ntuple.backward_train(eng, net, log, 1, 4, carousel=object())
    with pytest.raises(ValueError, match="tc or mean, not both"):
        ntuple.backward_train(eng, net, log, 1, 4, tc=ntuple.NTupleTC(net), mean=ntuple.NTupleMean(net))
    with pytest.raises(ValueError, match="log must be an NTupleLog of 8 boards"):
        ntuple.backward_train(eng, net, ntuple.NTupleLog(9, depth=2, device="cpu"), 1, 4)
    with pytest.raises(ValueError, match="mean must be the NTupleMean of this network"):
        ntuple.backward_train(eng, net, log, 1, 4, mean=ntuple.NTupleMean(other))
    assert "carousel" in ntuple.backward_train.__doc__
