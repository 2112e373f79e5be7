"""CPU: tile-downgrading (g2048_downgrade_plain, g2048_downgrade_boards, g2048_ntuple_play_downgraded and its staged sibling,
INTEGRATION.md §26) and optimistic initialisation at the library's and the Python layer's doors, without a GPU: the four
symbols are exported and bound, the struct has the header's layout, the ABI number has not moved, everything the library can
refuse without an engine or a device it refuses before it looks at either (every call here carries at least one argument that
must be refused, so none reaches a launch), and the Python layer raises its ValueErrors before any launch.  The first test
fails on the parent commit: the symbols do not exist there.  (The numpy-RNG engine's refusal needs an engine:
tests/test_gpu_ntuple_play_downgraded.py.)"""
import ctypes as C

import pytest

import __graft_entry__ as ge
from ntuple_helpers import TUPLES_17x4

WEIGHTS, BOARDS, OUT, MISSING, ACTIVE, LEFT, HIST, MOVES = 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000, 0x90000, 0xa0000   # never used
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


def _rule(min_exp=15, floor_exp=4):
    from gym2048_amd import _lib
    return _lib.DowngradeC(min_exp, floor_exp)


def refused(lib, rc, *words):
    msg = lib.g2048_last_error()
    assert rc == -1 and msg and all(w in msg for w in words), (rc, msg)


BAD_RULES = [((0, 4), b"min_exp=0"), ((32, 4), b"min_exp=32"), ((0xffffffff, 4), b"min_exp=4294967295"), ((15, 3), b"floor_exp=3"),
             ((15, 0), b"floor_exp=0"), ((15, 32), b"floor_exp=32")]
EDGE_RULES = [(1, 4), (31, 4), (15, 31), (31, 31)]


def test_symbols_are_exported_and_bound_and_the_abi_is_still_16(lib):
    from gym2048_amd import _lib
    d_p, io_p, u32, u64, P = C.POINTER(_lib.DowngradeC), C.POINTER(_lib.NTuplePlayIO), C.c_uint32, C.c_uint64, C.c_void_p
    want = {"g2048_downgrade_plain": [P, u64, d_p, P, P, P], "g2048_downgrade_boards": [P, d_p, P, P, P, P],
            "g2048_ntuple_play_downgraded": [P, C.POINTER(_lib.NTupleNetC), d_p, u32, io_p, P],
            "g2048_ntuple_staged_play_downgraded": [P, C.POINTER(_lib.NTupleStagedNetC), d_p, u32, io_p, P]}
    for name, argtypes in want.items():
        assert hasattr(lib, name), name
        assert _lib.SIGNATURES[name] == (C.c_int, argtypes), name
    assert lib.g2048_abi_version() == _lib.ABI_VERSION == 16
    assert [f[0] for f in _lib.DowngradeC._fields_] == ["min_exp", "floor_exp"] and C.sizeof(_lib.DowngradeC) == 8
    header = open(ge.os.path.join(ge.ROOT, "include", "g2048.h")).read()
    for line in ("#define G2048_DOWNGRADE_MIN_FLOOR 4", "#define G2048_DOWNGRADE_SKIPPED 0xff"):
        assert line in header
    init = open(ge.os.path.join(ge.PKG, "__init__.py")).read()
    for name in ("Downgrade", "Downgraded", "DowngradedPlayer", "downgrade"):
        assert f'"{name}"' in init                                          # exported by name (resolved on first use: needs torch)


def test_downgrade_plain_refusals_without_a_device(lib):
    plain = lambda r, boards=BOARDS, n=N, out=OUT, missing=MISSING: lib.g2048_downgrade_plain(boards, n, r, out, missing, None)  # noqa: E731
    refused(lib, plain(None), b"rule is NULL")
    for args, word in BAD_RULES:
        refused(lib, plain(C.byref(_rule(*args))), word)
    ok = C.byref(_rule())
    refused(lib, plain(ok, boards=None), b"boards is NULL")
    refused(lib, plain(ok, boards=BOARDS + 8), b"misaligned", b"boards need 16 bytes")
    refused(lib, plain(ok, out=None), b"out is NULL")
    refused(lib, plain(ok, out=OUT + 4), b"misaligned", b"out needs 16 bytes")
    refused(lib, plain(ok, n=0), b"n=0")
    refused(lib, plain(ok, n=0xffffff01), b"n=4294967041")
    refused(lib, plain(ok, n=1 << 32), b"n=4294967296")
    # the edges of both ranges are in range: what is refused then is the next thing wrong (missing may be NULL)
    for args in EDGE_RULES:
        refused(lib, plain(C.byref(_rule(*args)), out=None, missing=None), b"out is NULL")


def test_downgrade_boards_refusals_without_a_device(lib):
    boards = lambda e, r, active=ACTIVE, out=OUT: lib.g2048_downgrade_boards(e, r, active, out, MISSING, None)  # noqa: E731
    ok = C.byref(_rule())
    refused(lib, boards(None, ok), b"engine is NULL")                      # all in order but the engine
    refused(lib, boards(None, ok, active=None), b"engine is NULL")         # (active may be NULL)
    refused(lib, boards(None, None), b"rule is NULL")
    for args, word in BAD_RULES:
        refused(lib, boards(None, C.byref(_rule(*args))), word)
    refused(lib, boards(None, ok, out=None), b"out is NULL")
    refused(lib, boards(None, ok, out=OUT + 8), b"misaligned", b"out needs 16 bytes")
    refused(lib, boards(None, ok, active=ACTIVE + 2), b"misaligned", b"active needs 4 bytes")
    for args in EDGE_RULES:
        refused(lib, boards(None, C.byref(_rule(*args))), b"engine is NULL")


def test_play_downgraded_refusals_without_a_device(lib):
    from gym2048_amd import _lib
    for form in FORMS:
        staged = bool(form)
        net = _net(staged)
        play = lambda n, r, io=None, f=getattr(lib, "g2048_ntuple_" + form + "play_downgraded"): f(None, n, r, 4, io, None)   # noqa: E731
        ok = C.byref(_rule())
        refused(lib, play(C.byref(net), ok), b"engine is NULL")            # all in order but the engine
        refused(lib, play(None, ok), b"net is NULL")
        refused(lib, play(C.byref(net), None), b"rule is NULL")
        for args, word in BAD_RULES:
            refused(lib, play(C.byref(net), C.byref(_rule(*args))), word)
        for args in EDGE_RULES:
            refused(lib, play(C.byref(net), C.byref(_rule(*args))), b"engine is NULL")
        # what g2048_ntuple_play refuses is still refused
        bad = _net(staged)
        (bad.net if staged else bad).n_tuples = 9
        refused(lib, play(C.byref(bad), ok), b"n_tuples=9")
        for field, offset, words in (("games_left", 2, (b"misaligned", b"4 bytes")), ("hist", 4, (b"misaligned", b"8 bytes")),
                                     ("moves", 4, (b"misaligned", b"8 bytes"))):
            io = _lib.NTuplePlayIO(LEFT, HIST, MOVES)
            setattr(io, field, getattr(io, field) + offset)
            refused(lib, play(C.byref(net), ok, C.byref(io)), *words)
    # the entry point without a rule still does not ask for one
    refused(lib, lib.g2048_ntuple_play(None, C.byref(_net(False)), 4, None, None), b"engine is NULL")


def test_python_value_errors_before_any_launch():
    """The rule's ranges, the wrapped player's type, downgrade= with player=, and fill_value's overflow: raised before an engine or a
    device is looked at."""
    pytest.importorskip("torch")
    from gym2048_amd import ntuple
    rule = ntuple.Downgrade()
    assert (rule.min_tile, rule.floor_tile, rule._c.min_exp, rule._c.floor_exp) == (32768, 16, 15, 4)
    assert (ntuple.DOWNGRADE_MIN_FLOOR, ntuple.DOWNGRADE_SKIPPED) == (4, 0xff)
    edge = ntuple.Downgrade(2, 1 << 31)
    assert (edge._c.min_exp, edge._c.floor_exp) == (1, 31)
    for kw in (dict(min_tile=1), dict(min_tile=3), dict(min_tile=1 << 32), dict(min_tile=2048.0), dict(floor_tile=8), dict(floor_tile=24),
               dict(floor_tile=1 << 32), dict(min_tile=True)):
        with pytest.raises(ValueError):
            ntuple.Downgrade(**kw)
    with pytest.raises(ValueError, match="rule must be a Downgrade"):
        ntuple._rule((15, 4))
    with pytest.raises(ValueError, match="DeepPlayer"):
        ntuple.DowngradedPlayer(lambda engine, actions: None, rule)
    with pytest.raises(ValueError, match="wrap the player"):
        ntuple.play_games(None, None, player=lambda engine, actions: None, downgrade=rule)
    with pytest.raises(ValueError, match="Downgrade"):
        ntuple.play_games(None, ntuple.NTupleNet.__new__(ntuple.NTupleNet), downgrade=(15, 4))
    import inspect
    assert ntuple.play_games.__kwdefaults__ == {"downgrade": None}           # keyword only: the positional arguments stay what they were
    assert list(inspect.signature(ntuple.play_games).parameters) == ["engine", "net", "games", "chunk", "max_steps", "depth", "player"]
    assert inspect.signature(ntuple.NTupleNet.__init__).parameters["init_value"].default is None
    net = ntuple.NTupleNet("17x4", frac_bits=10, device="cpu")             # (a CPU tensor holds the weights: nothing is launched)
    assert net.fill_value(100000) is net
    assert net.weights.unique().tolist() == [(100000 << 10) // 40] and (100000 << 10) // 40 * 40 <= 100000 << 10
    net.fill_value(-7)
    assert net.weights.unique().tolist() == [(-7 << 10) // 40]              # floor division
    with pytest.raises(ValueError, match="does not fit in int32"):
        net.fill_value(1 << 27)                                            # (2^27 << 10) / 40 > 2^31
    assert net.weights.unique().tolist() == [(-7 << 10) // 40]              # a refused call changes nothing
    assert ntuple.NTupleNet("17x4", device="cpu", stages=(ntuple.stage_mask(2048),), init_value=8000).weights.unique().tolist() == [8000 * 1024 // 40]
