"""CPU: the expectimax entry points (g2048_expectimax, g2048_expectimax_plain) are exported, bound with a pinned struct
layout, refuse bad arguments with a message before touching a device, and leave the ABI version at 16 -- so these checks
run without a GPU."""
import ctypes as C
import os

import pytest

import __graft_entry__ as ge


@pytest.fixture(scope="module")
def lib():
    ge.build_hip()
    from gym2048_amd import _lib
    return _lib.load()


def _io(depth=2, base=4096, w_empty=256, w_merge=128, w_mono=16, action=None, value=None):
    from gym2048_amd import _lib
    return _lib.SearchIO(depth, base, w_empty, w_merge, w_mono, action, value)


def test_symbols_exported_and_bound(lib):
    from gym2048_amd import _lib
    for name in ("g2048_expectimax", "g2048_expectimax_plain"):
        assert hasattr(lib, name)
        assert name in _lib.SIGNATURES
    assert lib.g2048_abi_version() == _lib.ABI_VERSION == 16


def test_struct_layout():
    from gym2048_amd import _lib
    assert C.sizeof(_lib.SearchIO) == 40  # uint32 depth + four int32 weights, padded to 24, then two pointers
    assert [f[0] for f in _lib.SearchIO._fields_] == ["depth", "base", "w_empty", "w_merge", "w_mono", "action", "value"]
    assert (_lib.SearchIO.base.offset, _lib.SearchIO.w_mono.offset) == (4, 16)
    assert (_lib.SearchIO.action.offset, _lib.SearchIO.value.offset) == (24, 32)


def test_header_pins_the_defaults():
    from gym2048_amd.batched import SearchWeights  # noqa: F401  (torch is only needed for this import)
    text = open(os.path.join(ge.ROOT, "include", "g2048.h")).read()
    for name, v in (("BASE", 4096), ("EMPTY", 256), ("MERGE", 128), ("MONO", 16), ("MAX_DEPTH", 3)):
        assert f"#define G2048_SEARCH_{name} {v}\n" in text
    assert tuple(SearchWeights()) == (4096, 256, 128, 16)
    dev = open(os.path.join(ge.CSRC, "g2048_device.h")).read()
    assert "kSearchBase = 4096, kSearchEmpty = 256, kSearchMerge = 128, kSearchMono = 16" in dev


# fake device addresses: every case below is refused before the pointer could be used
BOARDS, OUT = 0x10000, 0x20000


@pytest.mark.parametrize("args, message", [
    ((None, 4, _io(action=OUT)), b"boards is NULL"),
    ((BOARDS + 8, 4, _io(action=OUT)), b"misaligned"),
    ((BOARDS, 0, _io(action=OUT)), b"n=0"),
    ((BOARDS, 1 << 32, _io(action=OUT)), b"n=4294967296"),
    ((BOARDS, 4, None), b"io is NULL"),
    ((BOARDS, 4, _io()), b"requests no output"),
    ((BOARDS, 4, _io(value=OUT + 4)), b"misaligned"),
    ((BOARDS, 4, _io(value=OUT + 8, action=OUT)), b"misaligned"),
    ((BOARDS, 4, _io(depth=0, action=OUT)), b"depth=0"),
    ((BOARDS, 4, _io(depth=4, value=OUT)), b"depth=4"),
    ((BOARDS, 4, _io(base=-1, action=OUT)), b"base=-1"),
    ((BOARDS, 4, _io(base=(1 << 24) + 1, action=OUT)), b"base=16777217"),
    ((BOARDS, 4, _io(w_empty=-1, action=OUT)), b"w_empty=-1"),
    ((BOARDS, 4, _io(w_merge=65536, action=OUT)), b"w_merge=65536"),
    ((BOARDS, 4, _io(w_mono=1 << 30, action=OUT)), b"w_mono=1073741824"),
])
def test_plain_form_argument_errors(lib, args, message):
    boards, n, io = args
    rc = lib.g2048_expectimax_plain(boards, n, None if io is None else C.byref(io), None)
    assert rc == -1
    assert message in lib.g2048_last_error()


def test_engine_form_needs_an_engine(lib):
    io = _io(action=OUT)
    assert lib.g2048_expectimax(None, C.byref(io), None) == -1
    assert b"engine is NULL" in lib.g2048_last_error()


def test_python_wrapper_checks_its_input():
    torch = pytest.importorskip("torch")
    import gym2048_amd
    from gym2048_amd import batched
    with pytest.raises(ValueError):
        gym2048_amd.expectimax(torch.zeros((4, 16), dtype=torch.uint8))         # host tensor: refused before the library
    with pytest.raises(ValueError):
        gym2048_amd.expectimax(torch.zeros((4, 15), dtype=torch.uint8))
    assert gym2048_amd.Search._fields == ("action", "value")
    assert gym2048_amd.SearchWeights._fields == ("base", "w_empty", "w_merge", "w_mono")
    cpu = torch.device("cpu")
    for depth in (0, 4, 2.0, True, None):
        with pytest.raises(ValueError, match="depth"):
            batched._search_io(4, cpu, depth, None, None)
    for w in ((-1, 0, 0, 0), ((1 << 24) + 1, 0, 0, 0), (0, 65536, 0, 0), (0, 0, 0, 1.5)):
        with pytest.raises(ValueError, match="weights"):
            batched._search_io(4, cpu, 2, w, None)
    with pytest.raises(ValueError, match="no output"):
        batched._search_io(4, cpu, 2, None, gym2048_amd.Search(None, None))
    with pytest.raises(ValueError, match="out.value"):
        batched._search_io(4, cpu, 2, None, gym2048_amd.Search(None, torch.zeros((4, 4), dtype=torch.int64)))
    io, out = batched._search_io(4, cpu, 3, (1, 2, 3, 4), None)
    assert (io.depth, io.base, io.w_empty, io.w_merge, io.w_mono) == (3, 1, 2, 3, 4)
    assert out.action.shape == (4,) and out.value.shape == (4, 4)
