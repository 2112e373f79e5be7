"""CPU: the budgeted play step and the masked search (g2048_play_step, g2048_ntuple_search_active) at the
library's and the Python layer's doors, without a GPU: the three symbols are exported and bound, the ABI number has not
moved, what the library can refuse without an engine it refuses before it looks at the engine (so a NULL engine shows
every such refusal here; the refusals that need a live engine -- numpy-RNG mode, and g2048_ntuple_search's own of the net
and the io -- are in test_gpu_play_step.py), the Python wrappers raise their ValueErrors before any launch, and the
reference of the budgeted step (play_step_helpers) reaches, from its own trace, what its inputs are there for."""
import ctypes as C
import types

import numpy as np
import pytest

import __graft_entry__ as ge
import ntuple_play_ref as pref
import play_step_helpers as psh
from ntuple_helpers import TUPLES_17x4

BUF, OUT, WEIGHTS = 0x10000, 0x20000, 0x30000      # fake device addresses: every call below is refused before they are used


@pytest.fixture(scope="module")
def lib():
    ge.build_hip()
    from gym2048_amd import _lib
    return _lib.load()


def _net():
    from gym2048_amd import _lib
    net = _lib.NTupleNetC(5, 4, 10)
    for t, cells in enumerate(TUPLES_17x4):
        for k, c in enumerate(cells):
            net.cells[t][k] = c
    net.weights = WEIGHTS
    return net


def test_symbols_are_exported_and_bound_and_the_abi_is_still_16(lib):
    from gym2048_amd import _lib
    io_p, search_p = C.POINTER(_lib.NTuplePlayIO), C.POINTER(_lib.NTupleSearchIO)
    want = {"g2048_play_step": [C.c_void_p, C.c_void_p, C.c_int32, io_p, C.c_void_p],
            "g2048_ntuple_search_active": [C.c_void_p, C.POINTER(_lib.NTupleNetC), search_p, C.c_void_p, C.c_void_p],
            "g2048_ntuple_staged_search_active": [C.c_void_p, C.POINTER(_lib.NTupleStagedNetC), search_p, C.c_void_p, C.c_void_p]}
    for name, argtypes in want.items():
        assert hasattr(lib, name)
        assert _lib.SIGNATURES[name] == (C.c_int, argtypes)
    assert lib.g2048_abi_version() == _lib.ABI_VERSION == 16


def refused(lib, rc, *words):
    msg = lib.g2048_last_error()
    assert rc == -1 and msg and all(w in msg for w in words), (rc, msg)


def test_play_step_refusals_without_a_device(lib):
    from gym2048_amd import _lib
    fn = lib.g2048_play_step
    good = _lib.NTuplePlayIO(OUT, OUT, OUT)
    for io in (None, C.byref(good)):
        for dtype, buf in ((_lib.ACT_RANDOM, None), (_lib.ACT_U8, BUF), (_lib.ACT_I32, BUF), (_lib.ACT_I64, BUF)):
            refused(lib, fn(None, buf, dtype, io, None), b"engine is NULL")
        for dtype in (_lib.ACT_U8, _lib.ACT_I32, _lib.ACT_I64):
            refused(lib, fn(None, None, dtype, io, None), b"actions is NULL")
        for dtype in (-1, 4, 1 << 20):
            refused(lib, fn(None, BUF, dtype, io, None), b"unknown action_dtype")
        for dtype, off in ((_lib.ACT_I32, 2), (_lib.ACT_I64, 4)):
            refused(lib, fn(None, BUF + off, dtype, io, None), b"misaligned", b"actions")
    for field, off in (("games_left", 2), ("hist", 4), ("moves", 4)):
        io = _lib.NTuplePlayIO(OUT, OUT, OUT)
        setattr(io, field, OUT + off)
        refused(lib, fn(None, BUF, _lib.ACT_U8, C.byref(io), None), b"misaligned", b"ntuple play")


@pytest.mark.parametrize("staged", (False, True), ids=("net", "staged_net"))
def test_search_active_refusals_without_a_device(lib, staged):
    from gym2048_amd import _lib
    fn = lib.g2048_ntuple_staged_search_active if staged else lib.g2048_ntuple_search_active
    net = _lib.NTupleStagedNetC(_net(), 1) if staged else _net()
    io = _lib.NTupleSearchIO(1, OUT, OUT)
    for active in (None, BUF):
        refused(lib, fn(None, C.byref(net), C.byref(io), active, None), b"engine is NULL")
        assert fn(None, None, None, active, None) == -1
    for off in (1, 2, 3):
        refused(lib, fn(None, C.byref(net), C.byref(io), BUF + off, None), b"misaligned", b"active")


def _engine(torch, n=8):
    """A Batched2048 that has no device behind it: enough for the checks that come before the library call."""
    from gym2048_amd.batched import Batched2048
    eng = Batched2048.__new__(Batched2048)
    eng._h, eng.n_envs, eng.device = None, n, torch.device("cpu")
    eng._lib = types.SimpleNamespace(g2048_destroy=lambda h: 0)
    return eng


def test_play_step_refuses_bad_arguments():
    import torch
    eng = _engine(torch)
    act = torch.zeros(8, dtype=torch.uint8)
    with pytest.raises(ValueError, match="actions must have shape"):
        eng.play_step(torch.zeros(9, dtype=torch.uint8))
    with pytest.raises(ValueError, match="actions must have shape"):
        eng.play_step(torch.zeros((1, 8), dtype=torch.uint8))
    with pytest.raises(TypeError, match="actions dtype"):                       # (step's own check, and its exception)
        eng.play_step(torch.zeros(8, dtype=torch.int16))
    good = dict(games_left=torch.zeros(8, dtype=torch.uint32), hist=torch.zeros(32, dtype=torch.uint64),
                moves=torch.zeros(1, dtype=torch.uint64))
    bad = dict(games_left=[torch.zeros(8, dtype=torch.int32), torch.zeros(9, dtype=torch.uint32), torch.zeros(16, dtype=torch.uint32)[::2]],
               hist=[torch.zeros(32, dtype=torch.int64), torch.zeros(31, dtype=torch.uint64)],
               moves=[torch.zeros(1, dtype=torch.int64), torch.zeros(2, dtype=torch.uint64)])
    for name, values in bad.items():
        for v in values:
            for actions in (act, None):
                with pytest.raises(ValueError, match=name + " must be a contiguous"):
                    eng.play_step(actions, **{**good, name: v})


def test_ntuple_search_refuses_a_bad_mask():
    import torch
    from gym2048_amd import ntuple
    eng, net = _engine(torch), ntuple.NTupleNet("17x4", device="cpu")
    for active in (torch.zeros(8, dtype=torch.int32), torch.zeros(9, dtype=torch.uint32), torch.zeros((8, 1), dtype=torch.uint32),
                   torch.zeros(16, dtype=torch.uint32)[::2], torch.zeros(8, dtype=torch.uint32, device="meta"), [1] * 8):
        with pytest.raises(ValueError, match="active must be a contiguous uint32"):
            eng.ntuple_search(net, 1, active=active)
    with pytest.raises(ValueError, match="net must be an NTupleNet"):
        eng.ntuple_search(object(), 1, active=torch.zeros(8, dtype=torch.uint32))
    with pytest.raises(ValueError, match="depth"):
        eng.ntuple_search(net, 3, active=torch.zeros(8, dtype=torch.uint32))


def test_play_games_checks_its_arguments_before_touching_the_engine():
    import torch
    from gym2048_amd import ntuple
    net = ntuple.NTupleNet("17x4", device="cpu")
    player = lambda e, a: None
    for kw in (dict(depth=-1), dict(depth=3), dict(depth=1.5), dict(depth=1, player=player), dict(depth=2, player=player),
               dict(player=3), dict(games=0, depth=1), dict(chunk=0, player=player), dict(max_steps=0, depth=2)):
        with pytest.raises(ValueError):
            ntuple.play_games(None, net, **kw)                  # (engine None: anything that touched it would be an AttributeError)
    for depth in (0, 1, 2):
        with pytest.raises(ValueError, match="net must be an NTupleNet"):
            ntuple.play_games(None, None, depth=depth)          # no player and no network
        with pytest.raises(ValueError, match="net must be an NTupleNet"):
            ntuple.play_games(None, object(), depth=depth)
    import inspect
    assert list(inspect.signature(ntuple.play_games).parameters) == ["engine", "net", "games", "chunk", "max_steps", "depth", "player"]
    assert ntuple.PlayReport._fields == ("games", "unfinished", "mean_score", "hist", "reach", "moves", "scores")


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("n", [65, 257])
def test_the_reference_reaches_what_its_inputs_are_for(n):
    actions, tr = psh.table_trace(n)
    budget = psh.budgets(n, 5)
    want = pref.limited(tr, budget)
    psh.assert_reaches(tr, want)                                # two episodes, an illegal end, all four directions, ran out, never moved
    assert actions.shape == (psh.K_TABLE, n) and set(np.unique(actions)) == {0, 1, 2, 3}
    # the budgeted form, restated per board: it plays exactly until its budget-th episode end, never past it
    for i in range(n):
        ends = np.nonzero(tr.terminated[:, i])[0]
        g = int(budget[i])
        last = tr.k if g > len(ends) else (ends[g - 1] + 1 if g else 0)
        assert want.played[:, i].sum() == last and want.played[:last, i].all()
        assert want.games_left[i] == g - min(g, len(ends))
    assert want.moves == int(want.played.sum()) and int(want.hist.sum()) == int(want.episodes.sum()) and want.clock == tr.t0 + tr.k
    assert (want.games_left[budget == pref.NO_LIMIT] > pref.NO_LIMIT - psh.K_TABLE).all()
    rest = ~want.played.any(axis=0)
    assert np.array_equal(want.records[rest], tr.start[rest]) and not want.last_records[rest].any()


def test_the_engineered_reference_reaches_the_late_game_cases():
    actions, tr = psh.engineered_table_trace()                  # (its assertions are inside)
    want = pref.limited(tr, psh.budgets(96, 6))
    hit = pref.reaches(tr, want)
    assert hit.illegal_end and hit.never_moved and hit.one_episode
