"""CPU: the fused n-tuple TD step and trainer (g2048_ntuple_td_step, g2048_ntuple_td_train and their staged siblings,
INTEGRATION.md §21) at the library's and the Python layer's doors, without a GPU: the four symbols are exported and bound, the
struct has the header's layout, the ABI number has not moved, everything the library can refuse without an engine it refuses
before it looks at the engine (so a NULL engine shows every such refusal here, with its message; the one refusal that needs
a live engine, numpy-RNG mode, is in test_gpu_ntuple_td.py), and the Python wrappers raise their ValueErrors before any
launch.  The first test fails on the parent commit: the symbols do not exist there."""
import ctypes as C
import types

import pytest

import __graft_entry__ as ge
from ntuple_helpers import TUPLES_17x4

BUF, OUT, WEIGHTS, ACC = 0x10000, 0x20000, 0x30000, 0x40000     # fake device addresses: every call below is refused before they are used
STEP = ("g2048_ntuple_td_step", "g2048_ntuple_staged_td_step")
TRAIN = ("g2048_ntuple_td_train", "g2048_ntuple_staged_td_train")


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


def _io(**kw):
    from gym2048_amd import _lib
    io = _lib.NTupleTDIO(OUT, OUT, OUT, OUT, OUT, OUT)
    for name, v in kw.items():
        setattr(io, name, v)
    return io


def refused(lib, rc, *words):
    msg = lib.g2048_last_error()
    assert rc == -1 and msg and all(w in msg for w in words), (rc, msg)


def test_symbols_are_exported_and_bound_and_the_abi_is_still_16(lib):
    from gym2048_amd import _lib
    io_p, tc_p, u32 = C.POINTER(_lib.NTupleTDIO), C.POINTER(_lib.NTupleTCC), C.c_uint32
    net_p, staged_p = C.POINTER(_lib.NTupleNetC), C.POINTER(_lib.NTupleStagedNetC)
    want = {"g2048_ntuple_td_step": [C.c_void_p, net_p, io_p, C.c_void_p],
            "g2048_ntuple_staged_td_step": [C.c_void_p, staged_p, io_p, C.c_void_p],
            "g2048_ntuple_td_train": [C.c_void_p, net_p, u32, u32, io_p, tc_p, C.c_void_p],
            "g2048_ntuple_staged_td_train": [C.c_void_p, staged_p, u32, u32, io_p, tc_p, C.c_void_p]}
    for name, argtypes in want.items():
        assert hasattr(lib, name)
        assert _lib.SIGNATURES[name] == (C.c_int, argtypes)
    assert lib.g2048_abi_version() == _lib.ABI_VERSION == 16
    assert [f[0] for f in _lib.NTupleTDIO._fields_] == ["action", "after", "after_value", "best_next", "terminated", "delta"]
    assert C.sizeof(_lib.NTupleTDIO) == 48


def calls(lib):
    """(name, staged, call(net, io) with a NULL engine) of the four entry points; the trainers at k_steps 3, lr_shift 4, TD(0)."""
    out = []
    for name in STEP:
        out.append((name, "staged" in name, lambda net, io, fn=getattr(lib, name): fn(None, net, io, None)))
    for name in TRAIN:
        out.append((name, "staged" in name, lambda net, io, fn=getattr(lib, name): fn(None, net, 3, 4, io, None, None)))
    return out


def test_refusals_without_a_device(lib):
    for name, staged, call in calls(lib):
        net = _net(staged)
        # everything in order but the engine
        refused(lib, call(C.byref(net), C.byref(_io())), b"engine is NULL")
        refused(lib, call(None, C.byref(_io())), b"net is NULL")
        refused(lib, call(C.byref(net), None), b"io is NULL")
        # a descriptor g2048_ntuple_evaluate refuses
        for field, value, word in (("n_tuples", 0, b"n_tuples=0"), ("n_tuples", 9, b"n_tuples=9"), ("tuple_len", 7, b"tuple_len=7"),
                                   ("frac_bits", 17, b"frac_bits=17"), ("weights", None, b"weights is NULL"),
                                   ("weights", WEIGHTS + 8, b"misaligned")):
            bad = _net(staged)
            setattr(bad.net if staged else bad, field, value)
            refused(lib, call(C.byref(bad), C.byref(_io())), word)
        bad = _net(staged)
        (bad.net if staged else bad).cells[1][2] = 16
        refused(lib, call(C.byref(bad), C.byref(_io())), b"cells[1][2]=16")
        if staged:
            bad = _net(True)
            bad.n_stages = 9
            refused(lib, call(C.byref(bad), C.byref(_io())), b"n_stages=9")
        # the outputs' alignment
        refused(lib, call(C.byref(net), C.byref(_io(after=OUT + 8))), b"misaligned", b"after needs 16 bytes")
        for field in ("after_value", "best_next", "delta"):
            refused(lib, call(C.byref(net), C.byref(_io(**{field: OUT + 4}))), b"misaligned", b"8 bytes")
        for field in ("action", "terminated"):                           # bytes: any address
            refused(lib, call(C.byref(net), C.byref(_io(**{field: OUT + 1}))), b"engine is NULL")


def test_step_takes_any_output_as_null(lib):
    """td_step has no required output: with any of them, or all of them, NULL the next refusal is the engine's."""
    for name in STEP:
        net = _net("staged" in name)
        fn = getattr(lib, name)
        for field in ("action", "after", "after_value", "best_next", "terminated", "delta"):
            refused(lib, fn(None, C.byref(net), C.byref(_io(**{field: None})), None), b"engine is NULL")
        from gym2048_amd import _lib
        refused(lib, fn(None, C.byref(net), C.byref(_lib.NTupleTDIO()), None), b"engine is NULL")


def test_train_refusals_without_a_device(lib):
    from gym2048_amd import _lib
    for name in TRAIN:
        net = _net("staged" in name)
        fn = getattr(lib, name)
        # (either descriptor's entry point names the unstaged symbol: one body serves both)
        refused(lib, fn(None, C.byref(net), 3, 4, C.byref(_io(after=None)), None, None), b"g2048_ntuple_td_train needs after and delta", b"after is NULL")
        refused(lib, fn(None, C.byref(net), 3, 4, C.byref(_io(delta=None)), None, None), b"g2048_ntuple_td_train needs after and delta", b"delta is NULL")
        for optional in ("action", "after_value", "best_next", "terminated"):
            refused(lib, fn(None, C.byref(net), 3, 4, C.byref(_io(**{optional: None})), None, None), b"engine is NULL")
        refused(lib, fn(None, C.byref(net), 3, 41, C.byref(_io()), None, None), b"lr_shift=41")
        refused(lib, fn(None, C.byref(net), 3, 40, C.byref(_io()), None, None), b"engine is NULL")
        # a tc g2048_ntuple_tc_update_plain refuses
        refused(lib, fn(None, C.byref(net), 3, 4, C.byref(_io()), C.byref(_lib.NTupleTCC(None, ACC)), None), b"tc err is NULL")
        refused(lib, fn(None, C.byref(net), 3, 4, C.byref(_io()), C.byref(_lib.NTupleTCC(ACC, None)), None), b"tc mag is NULL")
        refused(lib, fn(None, C.byref(net), 3, 4, C.byref(_io()), C.byref(_lib.NTupleTCC(ACC + 4, ACC)), None), b"misaligned", b"tc")
        refused(lib, fn(None, C.byref(net), 3, 4, C.byref(_io()), C.byref(_lib.NTupleTCC(ACC, ACC)), None), b"engine is NULL")
        # k_steps == 0 does not excuse a bad argument, and the engine is still looked at
        refused(lib, fn(None, C.byref(net), 0, 41, C.byref(_io()), None, None), b"lr_shift=41")
        refused(lib, fn(None, C.byref(net), 0, 4, C.byref(_io()), None, None), b"engine is NULL")


# ------------------------------------------------------------------------------------------------ the Python layer
def _engine(torch, n=8):
    """A Batched2048 that has no device behind it: enough for the checks that come before the library call."""
    from gym2048_amd.batched import Batched2048
    eng = Batched2048.__new__(Batched2048)
    eng._h, eng.n_envs, eng.device = None, n, torch.device("cpu")
    eng._lib = types.SimpleNamespace(g2048_destroy=lambda h: 0)
    eng.terminated = torch.zeros(n, dtype=torch.uint8)
    return eng


def test_python_wrappers_check_their_arguments_before_the_library():
    import torch
    from gym2048_amd import ntuple
    eng, net = _engine(torch), ntuple.NTupleNet("17x4", device="cpu")
    work = ntuple.td_work(eng)
    for call in (lambda **kw: eng.ntuple_td_step(**{"net": net, "work": work, **kw}),
                 lambda **kw: eng.ntuple_td_train(**{"net": net, "work": work, "n_steps": 1, "lr_shift": 4, **kw})):
        with pytest.raises(ValueError, match="net must be an NTupleNet"):
            call(net=object())
        with pytest.raises(ValueError, match="work must be a TDWork"):
            call(work=(work.before, work.after))
        with pytest.raises(ValueError, match="work delta must be a contiguous int64"):
            call(work=work._replace(delta=torch.zeros(8, dtype=torch.int32)))
        with pytest.raises(ValueError, match="work after must be a contiguous uint8"):
            call(work=work._replace(before=work.before._replace(after=torch.zeros((9, 16), dtype=torch.uint8))))
        with pytest.raises(ValueError, match="work best_next must be a contiguous int64"):
            call(work=work._replace(after=work.after._replace(best=None)))
    for kw in (dict(n_steps=-1), dict(n_steps=1 << 32), dict(n_steps=1.5), dict(lr_shift=41), dict(lr_shift=-1)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            eng.ntuple_td_train(**{"net": net, "work": work, "n_steps": 1, "lr_shift": 4, **kw})
    other = ntuple.NTupleNet("17x4", device="cpu")
    with pytest.raises(ValueError, match="tc must be the NTupleTC of this network"):
        eng.ntuple_td_train(net, work, 1, 4, tc=ntuple.NTupleTC(other))


def test_fused_with_a_carousel_is_refused_before_anything_runs():
    import inspect
    import torch
    from gym2048_amd import ntuple
    eng = _engine(torch)
    net = ntuple.NTupleNet("17x4", device="cpu", stages=(ntuple.stage_mask(8),))
    carousel = object()                                                  # (never looked at: the refusal comes first)
    work = ntuple.td_work(eng)
    calls = {"td_evaluate": (eng, net, work), "td_step": (eng, net, 4, work), "train": (eng, net, 2, 4),
             "tc_step": (eng, net, None, 4, work), "tc_train": (eng, net, None, 2, 4),
             "tdl_evaluate": (eng, net, None, work), "tdl_step": (eng, net, None, 4, work), "tdl_train": (eng, net, None, 2, 4),
             "tcl_step": (eng, net, None, None, 4, work), "tcl_train": (eng, net, None, None, 2, 4),
             "delayed_evaluate": (eng, net, None, work), "delayed_tdl_step": (eng, net, None, 4, work),
             "delayed_tdl_train": (eng, net, None, 2, 4), "delayed_tcl_step": (eng, net, None, None, 4, work),
             "delayed_tcl_train": (eng, net, None, None, 2, 4)}
    for name, args in calls.items():
        fn = getattr(ntuple, name)
        params = inspect.signature(fn).parameters
        assert params["fused"].default is False and list(params)[-2:] == ["carousel", "fused"], name
        if "delay" in name or name.startswith(("tdl", "tcl")):
            continue                                                     # (their history is checked first: a live one needs a device)
        with pytest.raises(ValueError, match="fused=True cannot run a carousel"):
            fn(*args, carousel=carousel, fused=True)
    assert "carousel" in ntuple.td_evaluate.__doc__ and "fused" in ntuple.td_evaluate.__doc__
