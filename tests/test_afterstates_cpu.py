"""CPU: the afterstate entry points (g2048_afterstates, g2048_afterstates_plain) are exported, bound with a pinned struct
layout, and refuse bad arguments with a message before touching a device -- so these checks run without a GPU."""
import ctypes as C

import pytest

import __graft_entry__ as ge


@pytest.fixture(scope="module")
def lib():
    ge.build_hip()
    from gym2048_amd import _lib
    return _lib.load()


def _io(boards=None, score=None, legal=None, obs=None, obs_dtype=0):
    from gym2048_amd import _lib
    return _lib.AfterstateIO(boards, score, legal, obs, obs_dtype)


def test_symbols_exported_and_bound(lib):
    from gym2048_amd import _lib
    for name in ("g2048_afterstates", "g2048_afterstates_plain"):
        assert hasattr(lib, name)
        assert name in _lib.SIGNATURES
    assert lib.g2048_abi_version() == _lib.ABI_VERSION == 16


def test_struct_layout():
    from gym2048_amd import _lib
    assert C.sizeof(_lib.AfterstateIO) == 40          # four pointers + int32 obs_dtype, padded to 8
    assert [f[0] for f in _lib.AfterstateIO._fields_] == ["boards", "score", "legal", "obs", "obs_dtype"]
    assert _lib.AfterstateIO.obs_dtype.offset == 32


# fake device addresses: every case below is refused before the pointer could be used
BOARDS, OUT = 0x10000, 0x20000


@pytest.mark.parametrize("args, message", [
    ((None, 4, _io(boards=OUT)), b"boards is NULL"),
    ((BOARDS + 8, 4, _io(boards=OUT)), b"misaligned"),
    ((BOARDS, 4, None), b"io is NULL"),
    ((BOARDS, 4, _io()), b"requests no output"),
    ((BOARDS, 4, _io(boards=OUT + 4)), b"misaligned"),
    ((BOARDS, 4, _io(score=OUT + 8)), b"misaligned"),
    ((BOARDS, 4, _io(obs=OUT + 1)), b"misaligned"),
    ((BOARDS, 4, _io(obs=OUT, obs_dtype=3)), b"unknown obs_dtype"),
    ((BOARDS, 4, _io(obs=OUT, obs_dtype=-1)), b"unknown obs_dtype"),
    ((BOARDS, 0, _io(boards=OUT)), b"n=0"),
    ((BOARDS, 1 << 32, _io(boards=OUT)), b"n=4294967296"),
])
def test_plain_form_argument_errors(lib, args, message):
    boards, n, io = args
    rc = lib.g2048_afterstates_plain(boards, n, None if io is None else C.byref(io), None)
    assert rc == -1
    assert message in lib.g2048_last_error()


def test_engine_form_needs_an_engine(lib):
    io = _io(boards=OUT)
    assert lib.g2048_afterstates(None, C.byref(io), None) == -1
    assert b"engine is NULL" in lib.g2048_last_error()


def test_python_wrapper_checks_its_input():
    torch = pytest.importorskip("torch")
    import gym2048_amd
    with pytest.raises(ValueError):
        gym2048_amd.afterstates(torch.zeros((4, 16), dtype=torch.uint8))         # host tensor: refused before the library
    with pytest.raises(ValueError):
        gym2048_amd.afterstates(torch.zeros((4, 15), dtype=torch.uint8))
    assert gym2048_amd.Afterstates._fields == ("boards", "score", "legal", "obs")
