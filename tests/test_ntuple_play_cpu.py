"""CPU: n-tuple play (g2048_ntuple_play) at the library's and the Python layer's doors, without a GPU:
the two symbols are exported and bound, the ABI number has not moved, a NULL engine or net is refused before any HIP call,
and the Python wrappers refuse what is not an NTupleNet and side outputs of the wrong dtype, shape, layout or device."""
import ctypes as C
import types

import pytest

import __graft_entry__ as ge
from ntuple_helpers import TUPLES_17x4

OUT, WEIGHTS = 0x20000, 0x30000      # fake device addresses: every call below is refused before they are used


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
    for name, net_type in (("g2048_ntuple_play", _lib.NTupleNetC), ("g2048_ntuple_staged_play", _lib.NTupleStagedNetC)):
        assert hasattr(lib, name)
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int and argtypes == [C.c_void_p, C.POINTER(net_type), C.c_uint32, C.POINTER(_lib.NTuplePlayIO), C.c_void_p]
    assert lib.g2048_abi_version() == _lib.ABI_VERSION == 16
    assert C.sizeof(_lib.NTuplePlayIO) == 24 and [f[0] for f in _lib.NTuplePlayIO._fields_] == ["games_left", "hist", "moves"]


@pytest.mark.parametrize("staged", (False, True), ids=("net", "staged_net"))
def test_null_engine_and_null_net_are_refused_without_a_device(lib, staged):
    from gym2048_amd import _lib
    fn = lib.g2048_ntuple_staged_play if staged else lib.g2048_ntuple_play
    net = _lib.NTupleStagedNetC(_net(), 1) if staged else _net()
    io = _lib.NTuplePlayIO(OUT, OUT, OUT)
    for k_steps in (0, 1, 1024):
        for io_ref in (None, C.byref(io)):
            assert fn(None, C.byref(net), k_steps, io_ref, None) == -1 and b"engine is NULL" in lib.g2048_last_error()
            assert fn(None, None, k_steps, io_ref, None) == -1


def _engine(torch, n=8):
    """A Batched2048 that has no device behind it: enough for the checks that come before the library call."""
    from gym2048_amd.batched import Batched2048
    eng = Batched2048.__new__(Batched2048)
    eng._h, eng.n_envs, eng.device = None, n, torch.device("cpu")
    eng._lib = types.SimpleNamespace(g2048_destroy=lambda h: 0)
    return eng


def test_python_wrapper_refuses_bad_arguments():
    import torch
    from gym2048_amd import ntuple
    eng, net = _engine(torch), ntuple.NTupleNet("17x4", device="cpu")
    with pytest.raises(ValueError, match="net must be an NTupleNet"):
        eng.ntuple_play(object(), 4)
    with pytest.raises(ValueError, match="k_steps"):
        eng.ntuple_play(net, -1)
    with pytest.raises(ValueError, match="k_steps"):
        eng.ntuple_play(net, 1 << 32)
    good = dict(games_left=torch.zeros(8, dtype=torch.uint32), hist=torch.zeros(32, dtype=torch.uint64),
                moves=torch.zeros(1, dtype=torch.uint64))
    bad = dict(games_left=[torch.zeros(8, dtype=torch.int32), torch.zeros(9, dtype=torch.uint32), torch.zeros((8, 1), dtype=torch.uint32),
                           torch.zeros(16, dtype=torch.uint32)[::2], [0] * 8],
               hist=[torch.zeros(32, dtype=torch.int64), torch.zeros(31, dtype=torch.uint64), torch.zeros(32, dtype=torch.uint32)],
               moves=[torch.zeros(1, dtype=torch.int64), torch.zeros((), dtype=torch.uint64), torch.zeros(2, dtype=torch.uint64)])
    for name, values in bad.items():
        for v in values:
            with pytest.raises(ValueError, match=name + " must be a contiguous"):
                eng.ntuple_play(net, 4, **{**good, name: v})
    with pytest.raises(ValueError, match="hist must be a contiguous"):
        ntuple._play_io(8, torch.device("meta"), None, good["hist"], None)      # the wrong device
    with pytest.raises(ValueError, match="the network's weights are on"):
        other = _engine(torch)
        other.device = torch.device("meta")
        other.ntuple_play(net, 4)
    io = ntuple._play_io(8, torch.device("cpu"), good["games_left"], None, good["moves"])
    assert io.games_left == good["games_left"].data_ptr() and io.hist is None and io.moves == good["moves"].data_ptr()


def test_play_games_checks_its_numbers_before_touching_the_engine():
    from gym2048_amd import ntuple
    for kw in (dict(games=0), dict(games=1 << 32), dict(chunk=0), dict(max_steps=0)):
        with pytest.raises(ValueError):
            ntuple.play_games(None, None, **kw)
    assert ntuple.PlayReport._fields == ("games", "unfinished", "mean_score", "hist", "reach", "moves", "scores")
    assert ntuple.REACH_TILES == (2048, 4096, 8192, 16384, 32768)
