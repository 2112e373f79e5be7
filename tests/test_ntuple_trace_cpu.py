"""CPU: the three g2048_ntuple_trace_* entry points exist, are bound, and validate every argument before any HIP call --
one case per message, without a device."""
import ctypes as C
import os

import pytest

import __graft_entry__ as ge
from ntuple_helpers import TUPLES_17x4

NAMES = ("g2048_ntuple_trace_push", "g2048_ntuple_trace_update", "g2048_ntuple_tc_trace_update")
# fake device addresses: every case below is refused before the pointer could be used
AFTER, VALUE, BEST, TERM, DELTA, WEIGHTS, HIST, LEN, ERR, MAG = (0x10000 * k for k in range(1, 11))


@pytest.fixture(scope="module")
def lib():
    ge.build_hip()
    from gym2048_amd import _lib
    return _lib.load()


def _net(T=5, weights=WEIGHTS):
    from gym2048_amd import _lib
    net = _lib.NTupleNetC(T, 4, 10)
    for t, cells in enumerate(TUPLES_17x4):
        for k, c in enumerate(cells):
            net.cells[t][k] = c
    net.weights = weights
    return C.byref(net)


def _tr(depth=4, lam=32768, hist=HIST, ln=LEN):
    from gym2048_amd import _lib
    return C.byref(_lib.NTupleTraceC(depth, lam, hist, ln))


def _tc(err=ERR, mag=MAG):
    from gym2048_amd import _lib
    return C.byref(_lib.NTupleTCC(err, mag))


def test_symbols_exported_and_abi_still_16(lib):
    from gym2048_amd import _lib
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.g2048_abi_version() == _lib.ABI_VERSION == 16


def test_struct_layout_and_header_limit():
    from gym2048_amd import _lib
    T = _lib.NTupleTraceC
    assert C.sizeof(T) == 24 and (T.depth.offset, T.lambda_.offset, T.hist.offset, T.len.offset) == (0, 4, 8, 16)
    assert "#define G2048_NTUPLE_TRACE_MAX 8\n" in open(os.path.join(ge.ROOT, "include", "g2048.h")).read()
    assert "kNtupleTraceMax = 8;" in open(os.path.join(ge.CSRC, "g2048_device.h")).read()


# the checks the three calls share: (keyword overrides of the trace, slot, message)
TRACE_ERRORS = [
    (None, 0, b"tr is NULL"),
    (dict(hist=None), 0, b"trace hist is NULL"),
    (dict(ln=None), 0, b"trace len is NULL"),
    (dict(depth=0), 0, b"depth=0"),
    (dict(depth=9), 0, b"depth=9"),
    (dict(lam=65537), 0, b"lambda=65537"),
    (dict(), 4, b"slot=4"),
    (dict(depth=1), 1, b"slot=1"),
    (dict(hist=HIST + 8), 0, b"trace hist needs 16 bytes"),
]


@pytest.mark.parametrize("kw, slot, message", TRACE_ERRORS, ids=[m.decode() for _, _, m in TRACE_ERRORS])
def test_trace_errors_in_every_entry_point(lib, kw, slot, message):
    tr = None if kw is None else _tr(**kw)
    for rc in (lib.g2048_ntuple_trace_push(AFTER, VALUE, BEST, TERM, 4, tr, slot, DELTA, None),
               lib.g2048_ntuple_trace_update(4, DELTA, 3, _net(), tr, slot, None),
               lib.g2048_ntuple_tc_trace_update(4, DELTA, 3, 3, _net(), _tc(), tr, slot, None)):
        assert rc == -1 and message in lib.g2048_last_error()


PUSH_ERRORS = [
    (dict(after=None), b"after is NULL"), (dict(value=None), b"after_value is NULL"), (dict(best=None), b"best_next is NULL"),
    (dict(term=None), b"terminated is NULL"), (dict(delta=None), b"delta is NULL"),
    (dict(n=0), b"n=0"), (dict(n=1 << 32), b"n=4294967296"),
    (dict(after=AFTER + 8), b"trace after needs 16 bytes"),
    (dict(value=VALUE + 4), b"after_value, best_next and delta need 8 bytes"),
    (dict(best=BEST + 4), b"after_value, best_next and delta need 8 bytes"),
    (dict(delta=DELTA + 4), b"after_value, best_next and delta need 8 bytes"),
]


@pytest.mark.parametrize("kw, message", PUSH_ERRORS, ids=[f"{list(k)[0]}: {m.decode()}" for k, m in PUSH_ERRORS])
def test_push_errors(lib, kw, message):
    a = dict(after=AFTER, value=VALUE, best=BEST, term=TERM, n=4, delta=DELTA)
    a.update(kw)
    assert lib.g2048_ntuple_trace_push(a["after"], a["value"], a["best"], a["term"], a["n"], _tr(), 0, a["delta"], None) == -1
    assert message in lib.g2048_last_error()


UPDATE_ERRORS = [
    (dict(net=None), b"net is NULL"), (dict(net=lambda: _net(T=9)), b"n_tuples=9"), (dict(net=lambda: _net(weights=None)), b"net weights is NULL"),
    (dict(n=0), b"n=0"), (dict(n=(1 << 32) - 255), b"n=4294967041"),
    (dict(delta=None), b"delta is NULL"), (dict(delta=DELTA + 4), b"ntuple delta needs 8 bytes"), (dict(shift=41), b"lr_shift=41"),
]


@pytest.mark.parametrize("kw, message", UPDATE_ERRORS, ids=[m.decode() for _, m in UPDATE_ERRORS])
def test_update_errors_in_both_updates(lib, kw, message):
    a = dict(n=4, delta=DELTA, shift=3, net=_net)
    a.update(kw)
    net = None if a["net"] is None else a["net"]()
    for rc in (lib.g2048_ntuple_trace_update(a["n"], a["delta"], a["shift"], net, _tr(), 0, None),
               lib.g2048_ntuple_tc_trace_update(a["n"], a["delta"], a["shift"], 3, net, _tc(), _tr(), 0, None)):
        assert rc == -1 and message in lib.g2048_last_error()


@pytest.mark.parametrize("phases, tc, message", [
    (0, _tc, b"phases=0"), (4, _tc, b"phases=4"), (3, None, b"tc is NULL"), (3, lambda: _tc(err=None), b"tc err is NULL"),
    (3, lambda: _tc(mag=None), b"tc mag is NULL"), (3, lambda: _tc(err=ERR + 4), b"err and mag need 8 bytes"),
    (3, lambda: _tc(mag=MAG + 4), b"err and mag need 8 bytes")])
def test_tc_errors(lib, phases, tc, message):
    assert lib.g2048_ntuple_tc_trace_update(4, DELTA, 3, phases, _net(), None if tc is None else tc(), _tr(), 0, None) == -1
    assert message in lib.g2048_last_error()
