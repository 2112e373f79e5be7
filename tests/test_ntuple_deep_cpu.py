"""CPU: the n-tuple deep search (g2048_ntuple_deep_search) at the library's and the Python layer's doors,
without a GPU: the header defines the constants and declares the four functions, they are exported and bound, the ABI number
has not moved, every argument the library can refuse it refuses before any HIP call (a NULL engine is refused first, so the
refusals behind a live engine are shown through the plain forms, which need none), the Python wrappers raise their ValueErrors
before any launch, and play_games hands the games left to a player that asks for them and to no other."""
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
NAMES = ("g2048_ntuple_deep_search", "g2048_ntuple_deep_search_plain", "g2048_ntuple_staged_deep_search",
         "g2048_ntuple_staged_deep_search_plain")


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


def refused(lib, rc, *words):
    msg = lib.g2048_last_error()
    assert rc == -1 and msg and all(w in msg for w in words), (rc, msg)


def test_the_header_defines_the_constants_and_declares_the_functions():
    text = header()
    defines = dict(re.findall(r"^#define (G2048_NTUPLE_DEEP_M\w+_DEPTH) (\d+)$", text, re.M))
    assert defines == {"G2048_NTUPLE_DEEP_MIN_DEPTH": "2", "G2048_NTUPLE_DEEP_MAX_DEPTH": "3"}
    assert re.search(r"^#define G2048_NTUPLE_SEARCH_MAX_DEPTH 2$", text, re.M), "the existing limit stays"
    for name in NAMES:
        assert len(re.findall(r"^int " + name + r"\(", text, re.M)) == 1, name
    struct = re.search(r"typedef struct g2048_ntuple_deep_io \{(.*?)\} g2048_ntuple_deep_io;", text, re.S).group(1)
    fields = re.findall(r"^\s+(?:const )?(\w+) \*?(\w+);", struct, re.M)
    assert fields == [("uint32_t", "depth"), ("uint8_t", "action"), ("int64_t", "value"), ("uint32_t", "active")]


def test_symbols_are_bound_and_the_constants_follow_the_header(lib):
    from gym2048_amd import _lib, ntuple
    io_p, net_p, staged_p = C.POINTER(_lib.NTupleDeepIO), C.POINTER(_lib.NTupleNetC), C.POINTER(_lib.NTupleStagedNetC)
    want = {NAMES[0]: [C.c_void_p, net_p, io_p, C.c_void_p], NAMES[1]: [C.c_void_p, C.c_uint64, net_p, io_p, C.c_void_p],
            NAMES[2]: [C.c_void_p, staged_p, io_p, C.c_void_p], NAMES[3]: [C.c_void_p, C.c_uint64, staged_p, io_p, C.c_void_p]}
    for name, argtypes in want.items():
        assert hasattr(lib, name)
        assert _lib.SIGNATURES[name] == (C.c_int, argtypes)
    assert [f for f, _ in _lib.NTupleDeepIO._fields_] == ["depth", "action", "value", "active"]
    defines = dict(re.findall(r"^#define (G2048_NTUPLE_\w+_DEPTH) (\d+)$", header(), re.M))
    assert ntuple.DEEP_MIN_DEPTH == int(defines["G2048_NTUPLE_DEEP_MIN_DEPTH"]) == 2
    assert ntuple.DEEP_MAX_DEPTH == int(defines["G2048_NTUPLE_DEEP_MAX_DEPTH"]) == 3
    assert ntuple.SEARCH_MAX_DEPTH == int(defines["G2048_NTUPLE_SEARCH_MAX_DEPTH"]) == 2
    assert lib.g2048_abi_version() == _lib.ABI_VERSION == 16


@pytest.mark.parametrize("staged", (False, True), ids=("net", "staged_net"))
def test_engine_forms_refuse_without_a_device(lib, staged):
    from gym2048_amd import _lib
    fn = getattr(lib, NAMES[2 if staged else 0])
    net, io = _net(staged), _lib.NTupleDeepIO(3, OUT, OUT, None)
    refused(lib, fn(None, C.byref(net), C.byref(io), None), b"engine is NULL")
    assert fn(None, None, None, None) == -1


@pytest.mark.parametrize("staged", (False, True), ids=("net", "staged_net"))
def test_plain_forms_refuse_every_bad_argument_without_a_device(lib, staged):
    from gym2048_amd import _lib
    fn = getattr(lib, NAMES[3 if staged else 1])
    net = _net(staged)
    inner = net.net if staged else net
    good = lambda: _lib.NTupleDeepIO(3, OUT, OUT, None)
    refused(lib, fn(None, 4, C.byref(net), C.byref(good()), None), b"boards is NULL")
    refused(lib, fn(BUF + 8, 4, C.byref(net), C.byref(good()), None), b"misaligned", b"boards")
    refused(lib, fn(BUF, 0, C.byref(net), C.byref(good()), None), b"n=0", b"1 <= n <= 2^32 - 256")
    refused(lib, fn(BUF, 0xffffff01, C.byref(net), C.byref(good()), None), b"n=4294967041")
    refused(lib, fn(BUF, 4, None, C.byref(good()), None), b"net is NULL")
    refused(lib, fn(BUF, 4, C.byref(net), None, None), b"io is NULL")
    # the network checks of the other n-tuple calls, through the same functions
    inner.n_tuples = 9
    refused(lib, fn(BUF, 4, C.byref(net), C.byref(good()), None), b"n_tuples=9")
    inner.n_tuples = 5
    inner.frac_bits = 17
    refused(lib, fn(BUF, 4, C.byref(net), C.byref(good()), None), b"frac_bits=17")
    inner.frac_bits = 10
    inner.weights = None
    refused(lib, fn(BUF, 4, C.byref(net), C.byref(good()), None), b"weights")
    inner.weights = WEIGHTS
    inner.cells[1][2] = inner.cells[1][1]
    assert fn(BUF, 4, C.byref(net), C.byref(good()), None) == -1                # a cell twice in one tuple
    inner.cells[1][2] = 6
    if staged:
        net.n_stages = 9
        refused(lib, fn(BUF, 4, C.byref(net), C.byref(good()), None), b"n_stages=9")
        net.n_stages = 2
        net.thresholds[0] = 0
        assert fn(BUF, 4, C.byref(net), C.byref(good()), None) == -1            # a threshold of 0
        net.n_stages = 1
    # the io
    refused(lib, fn(BUF, 4, C.byref(net), C.byref(_lib.NTupleDeepIO(3, None, None, None)), None), b"requests no output")
    refused(lib, fn(BUF, 4, C.byref(net), C.byref(_lib.NTupleDeepIO(3, OUT, OUT + 8, None)), None), b"misaligned", b"value", b"16 bytes")
    for depth in (0, 1, 4, 1 << 31):
        refused(lib, fn(BUF, 4, C.byref(net), C.byref(_lib.NTupleDeepIO(depth, OUT, OUT, None)), None),
                b"depth=%d: need 2 <= depth <= 3" % depth)
    refused(lib, fn(BUF, 4, C.byref(net), C.byref(_lib.NTupleDeepIO(3, OUT, OUT, BUF)), None), b"active", b"plain form")
    # and the existing entry point still stops at depth 2
    old = getattr(lib, "g2048_ntuple_staged_search_plain" if staged else "g2048_ntuple_search_plain")
    refused(lib, old(BUF, 4, C.byref(net), C.byref(_lib.NTupleSearchIO(3, OUT, OUT)), None), b"depth=3: need 1 <= depth <= 2")


def _engine(torch, n=8):
    """A Batched2048 that has no device behind it: enough for the checks that come before the library call."""
    from gym2048_amd.batched import Batched2048
    eng = Batched2048.__new__(Batched2048)
    eng._h, eng.n_envs, eng.device = None, n, torch.device("cpu")
    eng._lib = types.SimpleNamespace(g2048_destroy=lambda h: 0)
    return eng


def test_python_argument_checks():
    import torch
    from gym2048_amd import ntuple
    net, eng = ntuple.NTupleNet("17x4", device="cpu"), _engine(torch)
    # NTupleNet.deep_search wants boards on a GPU first; its other checks are _deep_io's, which the engine method shares
    calls = (lambda depth=3, out=None: ntuple._deep_io(8, torch.device("cpu"), depth, out), lambda **kw: eng.ntuple_deep_search(net, **kw))
    with pytest.raises(ValueError, match="boards must be"):
        net.deep_search(torch.zeros((8, 16), dtype=torch.uint8))
    for call in calls:
        for depth in (1, 4, 0, -1, True, 1.0, 3.0, "3", None):
            with pytest.raises(ValueError, match="depth"):
                call(depth=depth)
        for out in ((torch.zeros(8, dtype=torch.int32), None), (torch.zeros(9, dtype=torch.uint8), None),
                    (None, torch.zeros((8, 4), dtype=torch.int32)), (None, torch.zeros((4, 8), dtype=torch.int64)),
                    (torch.zeros(16, dtype=torch.uint8)[::2], None)):
            with pytest.raises(ValueError, match="must be a contiguous"):
                call(depth=3, out=out)
        with pytest.raises(ValueError, match="no output"):
            call(depth=2, out=(None, None))
    for active in (torch.zeros(8, dtype=torch.int32), torch.zeros(9, dtype=torch.uint32), torch.zeros((8, 1), dtype=torch.uint32),
                   torch.zeros(16, dtype=torch.uint32)[::2], [1] * 8):
        with pytest.raises(ValueError, match="active must be a contiguous uint32"):
            eng.ntuple_deep_search(net, 3, active=active)
    with pytest.raises(ValueError, match="net must be an NTupleNet"):
        eng.ntuple_deep_search(object())
    assert "active" not in inspect.signature(net.deep_search).parameters            # plain boards take no mask
    assert inspect.signature(net.deep_search).parameters["depth"].default == 3
    assert inspect.signature(eng.ntuple_deep_search).parameters["depth"].default == 3


def test_deep_player():
    import gym2048_amd
    from gym2048_amd import ntuple
    assert gym2048_amd.DeepPlayer is ntuple.DeepPlayer and ntuple.DeepPlayer.takes_active is True
    net = ntuple.NTupleNet("17x4", device="cpu")
    assert ntuple.DeepPlayer(net).depth == 3 and ntuple.DeepPlayer(net, 2).depth == 2
    for depth in (1, 4, True, 2.0):
        with pytest.raises(ValueError, match="depth"):
            ntuple.DeepPlayer(net, depth)
    with pytest.raises(ValueError, match="net must be an NTupleNet"):
        ntuple.DeepPlayer(None)
    calls = []
    eng = types.SimpleNamespace(ntuple_deep_search=lambda *a, **kw: calls.append((a, kw)))
    ntuple.DeepPlayer(net, 2)(eng, "actions", active="left")
    ntuple.DeepPlayer(net)(eng, "actions")
    assert calls == [((net, 2), dict(out=ntuple.NTupleSearch("actions", None), active="left")),
                     ((net, 3), dict(out=ntuple.NTupleSearch("actions", None), active=None))]


class StubEngine:
    """What play_games touches, on the CPU: every board's one game ends at its third play_step."""

    def __init__(self, torch, n=4):
        self.torch, self.n_envs, self.device, self.last_records_enabled = torch, n, torch.device("cpu"), False
        self.steps = self.episodes = 0

    def reset(self):
        self.steps = 0

    def episode_stats(self):
        return {"episodes": self.episodes, "return_sum": 100 * self.episodes}

    def play_step(self, actions, games_left=None, hist=None, moves=None):
        self.steps += 1
        if self.steps == 3:
            self.episodes += self.n_envs
            games_left.view(self.torch.int32).zero_()


def test_play_games_gives_the_games_left_to_a_player_that_takes_them():
    import torch
    from gym2048_amd import ntuple
    seen = []

    class Taker:
        takes_active = True

        def __call__(self, engine, actions, active=None):
            seen.append(("taker", actions.dtype, tuple(actions.shape), active.dtype, active.view(torch.int32).tolist()))

    def plain(engine, actions):                       # a plain callable: two arguments, as before
        seen.append(("plain", actions.dtype, tuple(actions.shape)))

    class Refuser:                                    # the attribute present and false: called as a plain player
        takes_active = False

        def __call__(self, engine, actions):
            seen.append(("refuser",))

    report = ntuple.play_games(StubEngine(torch), None, games=1, chunk=3, player=Taker())
    assert seen == [("taker", torch.uint8, (4,), torch.uint32, [1] * 4)] * 3
    assert report.games == 4 and report.unfinished == 0 and report.mean_score == 100.0
    del seen[:]
    ntuple.play_games(StubEngine(torch), None, games=1, chunk=3, player=plain)
    ntuple.play_games(StubEngine(torch), None, games=1, chunk=3, player=Refuser())
    assert seen == [("plain", torch.uint8, (4,))] * 3 + [("refuser",)] * 3


def test_play_games_keeps_its_signature_and_its_depth_limit():
    from gym2048_amd import ntuple
    assert list(inspect.signature(ntuple.play_games).parameters) == ["engine", "net", "games", "chunk", "max_steps", "depth", "player"]
    assert [p.default for p in inspect.signature(ntuple.play_games).parameters.values()][2:] == [1, 1024, None, 0, None]
    net = ntuple.NTupleNet("17x4", device="cpu")
    with pytest.raises(ValueError, match="depth"):
        ntuple.play_games(None, net, depth=3)
    with pytest.raises(ValueError, match="depth=2 with a player"):
        ntuple.play_games(None, net, depth=2, player=ntuple.DeepPlayer(net))
