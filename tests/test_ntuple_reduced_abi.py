"""CPU: the n-tuple reduced search (g2048_ntuple_reduced_search) at the library's and the Python layer's
doors, without a GPU: the header defines the constants and declares the four functions, they are exported and bound with the
structure the header lays out, the ABI number has not moved, every argument the library can refuse it refuses before any HIP call
with its message (a NULL engine is refused first, so the refusals behind a live engine are shown through the plain forms, which
need none), and the Python wrappers raise their ValueErrors before any launch."""
import ctypes as C
import inspect
import os
import re
import types

import pytest

import __graft_entry__ as ge
from ntuple_helpers import TUPLES_17x4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUF, OUT, WEIGHTS = 0x10000, 0x20000, 0x30000      # fake device addresses: every call below is refused before they are used
NAMES = ("g2048_ntuple_reduced_search", "g2048_ntuple_reduced_search_plain", "g2048_ntuple_staged_reduced_search",
         "g2048_ntuple_staged_reduced_search_plain")
THREE = (3, 3, 3, 3, 3, 3, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1)        # "3-ply-late", written out
FOUR = (4, 4, 3, 3, 3, 3, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1)         # "4-ply-late"


@pytest.fixture(scope="module")
def lib():
    ge.build_hip()
    from gym2048_amd import _lib
    return _lib.load()


def header():
    with open(os.path.join(ROOT, "include", "g2048.h")) as f:
        return f.read()


def _net(staged=False):
    from gym2048_amd import _lib
    net = _lib.NTupleNetC(5, 4, 10)
    for t, cells in enumerate(TUPLES_17x4):
        for k, c in enumerate(cells):
            net.cells[t][k] = c
    net.weights = WEIGHTS
    return _lib.NTupleStagedNetC(net, 1) if staged else net


def _io(schedule=THREE, reduce4=1, action=OUT, value=OUT, depth=None, active=None):
    from gym2048_amd import _lib
    return _lib.NTupleReducedIO((C.c_uint8 * 17)(*schedule), reduce4, action, value, depth, active)


def refused(lib, rc, *words):
    msg = lib.g2048_last_error()
    assert rc == -1 and msg and all(w in msg for w in words), (rc, msg)


def test_the_header_defines_the_constants_and_declares_the_functions():
    text = header()
    assert re.search(r"^#define G2048_NTUPLE_REDUCE4_MIN 1$", text, re.M) and re.search(r"^#define G2048_NTUPLE_REDUCE4_MAX 2$", text, re.M)
    assert re.search(r"^#define G2048_NTUPLE_ADAPTIVE_MAX_DEPTH 4$", text, re.M), "the existing limit stays"
    for name in NAMES:
        assert len(re.findall(r"^int " + name + r"\(", text, re.M)) == 1, name
    struct = re.search(r"typedef struct g2048_ntuple_reduced_io \{(.*?)\} g2048_ntuple_reduced_io;", text, re.S).group(1)
    fields = re.findall(r"^\s+(?:const )?(\w+) \*?(\w+)(?:\[17\])?;", struct, re.M)
    assert fields == [("uint8_t", "schedule"), ("uint32_t", "reduce4"), ("uint8_t", "action"), ("int64_t", "value"), ("uint8_t", "depth"),
                      ("uint32_t", "active")]
    assert "uint8_t schedule[17];" in struct and "uint32_t reduce4;" in struct


def test_symbols_are_bound_and_the_layout_follows_the_header(lib):
    from gym2048_amd import _lib, ntuple
    io_p, net_p, staged_p = C.POINTER(_lib.NTupleReducedIO), C.POINTER(_lib.NTupleNetC), C.POINTER(_lib.NTupleStagedNetC)
    want = {NAMES[0]: [C.c_void_p, net_p, io_p, C.c_void_p], NAMES[1]: [C.c_void_p, C.c_uint64, net_p, io_p, C.c_void_p],
            NAMES[2]: [C.c_void_p, staged_p, io_p, C.c_void_p], NAMES[3]: [C.c_void_p, C.c_uint64, staged_p, io_p, C.c_void_p]}
    for name, argtypes in want.items():
        assert hasattr(lib, name)
        assert _lib.SIGNATURES[name] == (C.c_int, argtypes)
    assert [f for f, _ in _lib.NTupleReducedIO._fields_] == ["schedule", "reduce4", "action", "value", "depth", "active"]
    # the C layout: 17 bytes, the uint32 at its own alignment, then pointers at theirs
    io = _lib.NTupleReducedIO
    assert (io.schedule.offset, io.reduce4.offset, io.action.offset, io.value.offset, io.depth.offset, io.active.offset) == (0, 20, 24, 32, 40, 48)
    assert C.sizeof(io) == 56
    assert ntuple.REDUCE4_MIN == 1 and ntuple.REDUCE4_MAX == 2 and ntuple.ADAPTIVE_MAX_DEPTH == 4
    assert lib.g2048_abi_version() == _lib.ABI_VERSION == 16


@pytest.mark.parametrize("staged", (False, True), ids=("net", "staged_net"))
def test_engine_forms_refuse_without_a_device(lib, staged):
    fn = getattr(lib, NAMES[2 if staged else 0])
    net, io = _net(staged), _io()
    refused(lib, fn(None, C.byref(net), C.byref(io), None), b"engine is NULL")
    assert fn(None, None, None, None) == -1


@pytest.mark.parametrize("staged", (False, True), ids=("net", "staged_net"))
def test_plain_forms_refuse_every_bad_argument_without_a_device(lib, staged):
    fn = getattr(lib, NAMES[3 if staged else 1])
    net = _net(staged)
    inner = net.net if staged else net
    refused(lib, fn(None, 4, C.byref(net), C.byref(_io()), None), b"boards is NULL")
    refused(lib, fn(BUF + 8, 4, C.byref(net), C.byref(_io()), None), b"misaligned", b"boards")
    refused(lib, fn(BUF, 0, C.byref(net), C.byref(_io()), None), b"n=0", b"1 <= n <= 2^32 - 256")
    refused(lib, fn(BUF, 0xffffff01, C.byref(net), C.byref(_io()), None), b"n=4294967041")
    refused(lib, fn(BUF, 4, None, C.byref(_io()), None), b"net is NULL")
    refused(lib, fn(BUF, 4, C.byref(net), None, None), b"io is NULL")
    # a descriptor that g2048_ntuple_evaluate refuses
    inner.n_tuples = 9
    refused(lib, fn(BUF, 4, C.byref(net), C.byref(_io()), None), b"n_tuples=9")
    inner.n_tuples = 5
    inner.frac_bits = 17
    refused(lib, fn(BUF, 4, C.byref(net), C.byref(_io()), None), b"frac_bits=17")
    inner.frac_bits = 10
    inner.weights = None
    refused(lib, fn(BUF, 4, C.byref(net), C.byref(_io()), None), b"weights")
    inner.weights = WEIGHTS
    inner.cells[1][2] = inner.cells[1][1]
    assert fn(BUF, 4, C.byref(net), C.byref(_io()), None) == -1                # a cell twice in one tuple
    inner.cells[1][2] = 6
    if staged:
        net.n_stages = 9
        refused(lib, fn(BUF, 4, C.byref(net), C.byref(_io()), None), b"n_stages=9")
        net.n_stages = 2
        net.thresholds[0] = 0
        assert fn(BUF, 4, C.byref(net), C.byref(_io()), None) == -1            # a threshold of 0
        net.n_stages = 1
    # the io: the reduction, the schedule, the outputs, the mask
    refused(lib, fn(BUF, 4, C.byref(net), C.byref(_io(reduce4=0)), None), b"reduce4=0", b"1 <= reduce4 <= 2", b"g2048_ntuple_adaptive_search")
    for r in (3, 255, 0xffffffff):
        refused(lib, fn(BUF, 4, C.byref(net), C.byref(_io(reduce4=r)), None), b"reduce4=%d" % r, b"1 <= reduce4 <= 2")
    for e in (0, 7, 16):
        for d in (5, 255):
            bad = list(THREE)
            bad[e] = d
            refused(lib, fn(BUF, 4, C.byref(net), C.byref(_io(bad)), None), b"schedule[%d]=%d" % (e, d), b"0..4")
    for r in (1, 2):
        refused(lib, fn(BUF, 4, C.byref(net), C.byref(_io(reduce4=r, action=None, value=None)), None), b"g2048_ntuple_reduced_io",
                b"requests no output")
    refused(lib, fn(BUF, 4, C.byref(net), C.byref(_io(action=None, value=None, depth=OUT)), None), b"requests no output")
    refused(lib, fn(BUF, 4, C.byref(net), C.byref(_io(value=OUT + 8)), None), b"misaligned", b"reduced search value", b"16 bytes")
    refused(lib, fn(BUF, 4, C.byref(net), C.byref(_io(active=BUF)), None), b"g2048_ntuple_reduced_io active", b"plain form")
    # the adaptive entry points, which share the body, keep their own messages
    from gym2048_amd import _lib
    old = getattr(lib, "g2048_ntuple_staged_adaptive_search_plain" if staged else "g2048_ntuple_adaptive_search_plain")
    sched = (C.c_uint8 * 17)(*THREE)
    refused(lib, old(BUF, 4, C.byref(net), C.byref(_lib.NTupleAdaptiveIO(sched, None, None, None, None)), None),
            b"g2048_ntuple_adaptive_io requests no output")
    refused(lib, old(BUF, 4, C.byref(net), C.byref(_lib.NTupleAdaptiveIO(sched, OUT, OUT + 8, None, None)), None),
            b"ntuple adaptive search value needs 16 bytes")


def _engine(torch, n=8):
    """A Batched2048 that has no device behind it: enough for the checks that come before the library call."""
    from gym2048_amd.batched import Batched2048
    eng = Batched2048.__new__(Batched2048)
    eng._h, eng.n_envs, eng.device = None, n, torch.device("cpu")
    eng._lib = types.SimpleNamespace(g2048_destroy=lambda h: 0)
    return eng


def test_python_argument_checks():
    import torch
    from gym2048_amd import _lib, ntuple
    net, eng = ntuple.NTupleNet("17x4", device="cpu"), _engine(torch)
    calls = (lambda schedule=THREE, reduce4=1, out=None: ntuple._adaptive_io(8, torch.device("cpu"), schedule, out, reduce4=reduce4),
             lambda schedule=THREE, reduce4=1, **kw: eng.ntuple_reduced_search(net, schedule, reduce4, **kw))
    with pytest.raises(ValueError, match="boards must be"):
        net.reduced_search(torch.zeros((8, 16), dtype=torch.uint8), THREE)
    for call in calls:
        for schedule in (THREE[:16], THREE + (1,), (), 3, None, "5-ply", THREE[:16] + (5,), (-1,) + THREE[1:], THREE[:16] + (1.0,)):
            with pytest.raises(ValueError, match="schedule"):
                call(schedule=schedule)
        for reduce4 in (0, 3, -1, 1.0, True, "1"):
            with pytest.raises(ValueError, match="reduce4"):
                call(reduce4=reduce4)
        for out in ((torch.zeros(8, dtype=torch.int32), None, None), (None, torch.zeros((4, 8), dtype=torch.int64), None),
                    (torch.zeros(8, dtype=torch.uint8), None, torch.zeros(7, dtype=torch.uint8))):
            with pytest.raises(ValueError, match="must be a contiguous"):
                call(out=out)
        for out in ((None, None, None), (None, None, torch.zeros(8, dtype=torch.uint8))):
            with pytest.raises(ValueError, match="no output"):
                call(out=out)
    io, out = ntuple._adaptive_io(8, torch.device("cpu"), "4-ply-late", None, reduce4=2)
    assert isinstance(io, _lib.NTupleReducedIO) and tuple(io.schedule) == FOUR and io.reduce4 == 2
    assert out.action.dtype == out.depth.dtype == torch.uint8 and tuple(out.value.shape) == (8, 4)
    assert isinstance(ntuple._adaptive_io(8, torch.device("cpu"), THREE, None)[0], _lib.NTupleAdaptiveIO), "the adaptive io stays"
    for active in (torch.zeros(8, dtype=torch.int32), torch.zeros(9, dtype=torch.uint32), [1] * 8):
        with pytest.raises(ValueError, match="active must be a contiguous uint32"):
            eng.ntuple_reduced_search(net, THREE, active=active)
    with pytest.raises(ValueError, match="net must be an NTupleNet"):
        eng.ntuple_reduced_search(object(), THREE)
    assert list(inspect.signature(net.reduced_search).parameters) == ["boards", "schedule", "reduce4", "out"]
    assert list(inspect.signature(eng.ntuple_reduced_search).parameters) == ["net", "schedule", "reduce4", "out", "active"]
    assert inspect.signature(net.reduced_search).parameters["reduce4"].default == 1
    assert inspect.signature(eng.ntuple_reduced_search).parameters["reduce4"].default == 1


def test_reduced_player():
    import gym2048_amd
    from gym2048_amd import ntuple
    assert gym2048_amd.ReducedPlayer is ntuple.ReducedPlayer and ntuple.ReducedPlayer.takes_active is True
    net = ntuple.NTupleNet("17x4", device="cpu")
    p = ntuple.ReducedPlayer(net, "4-ply-late")
    assert p.schedule == FOUR and p.reduce4 == 1 and ntuple.ReducedPlayer(net, list(THREE), 2).reduce4 == 2
    for schedule in ("deep", THREE[:5], (5,) * 17, None):
        with pytest.raises(ValueError, match="schedule"):
            ntuple.ReducedPlayer(net, schedule)
    for reduce4 in (0, 3, None, 1.5):
        with pytest.raises(ValueError, match="reduce4"):
            ntuple.ReducedPlayer(net, THREE, reduce4)
    with pytest.raises(ValueError, match="net must be an NTupleNet"):
        ntuple.ReducedPlayer(None, THREE)
    calls = []
    eng = types.SimpleNamespace(ntuple_reduced_search=lambda *a, **kw: calls.append((a, kw)))
    ntuple.ReducedPlayer(net, "3-ply-late")(eng, "actions", active="left")
    ntuple.ReducedPlayer(net, FOUR, 2)(eng, "actions")
    assert calls == [((net, THREE, 1), dict(out=ntuple.NTupleAdaptive("actions", None, None), active="left")),
                     ((net, FOUR, 2), dict(out=ntuple.NTupleAdaptive("actions", None, None), active=None))]
    # play_games and the presets are unchanged
    assert list(inspect.signature(ntuple.play_games).parameters) == ["engine", "net", "games", "chunk", "max_steps", "depth", "player"]
    assert set(ntuple.SCHEDULES) == {"3-ply-late", "4-ply-late"}
