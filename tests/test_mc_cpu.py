"""CPU: the Monte-Carlo search entry points (g2048_mc_search, g2048_mc_search_plain) are exported, bound with a pinned
struct layout, refuse bad arguments with a message before touching a device, and leave the ABI version at 16 -- so these
checks run without a GPU."""
import ctypes as C
import os

import pytest

import __graft_entry__ as ge


@pytest.fixture(scope="module")
def lib():
    ge.build_hip()
    from gym2048_amd import _lib
    return _lib.load()


def _io(rollouts=64, max_steps=100, seed=0, action=None, value=None, steps=None):
    from gym2048_amd import _lib
    return _lib.MCIO(rollouts, max_steps, seed, action, value, steps)


def test_symbols_exported_and_bound(lib):
    from gym2048_amd import _lib
    for name in ("g2048_mc_search", "g2048_mc_search_plain"):
        assert hasattr(lib, name)
        assert name in _lib.SIGNATURES
    assert lib.g2048_abi_version() == _lib.ABI_VERSION == 16


def test_struct_layout():
    from gym2048_amd import _lib
    assert C.sizeof(_lib.MCIO) == 40  # two uint32, a uint64, three pointers
    assert [f[0] for f in _lib.MCIO._fields_] == ["rollouts", "max_steps", "seed", "action", "value", "steps"]
    assert (_lib.MCIO.rollouts.offset, _lib.MCIO.max_steps.offset, _lib.MCIO.seed.offset) == (0, 4, 8)
    assert (_lib.MCIO.action.offset, _lib.MCIO.value.offset, _lib.MCIO.steps.offset) == (16, 24, 32)


def test_header_pins_the_limits_and_the_key_tag():
    text = open(os.path.join(ge.ROOT, "include", "g2048.h")).read()
    assert "#define G2048_MC_MAX_ROLLOUTS 65536\n" in text and "#define G2048_MC_MAX_STEPS 65535\n" in text
    assert "seed_hi ^ 0x4D435332" in text
    dev = open(os.path.join(ge.CSRC, "g2048_device.h")).read()
    assert "kMcKeyTag = 0x4D435332u" in dev and "kMcMaxRollouts = 65536, kMcMaxSteps = 65535" in dev


# fake device addresses: every case below is refused before the pointer could be used
BOARDS, OUT = 0x10000, 0x20000


@pytest.mark.parametrize("args, message", [
    ((None, 4, 0, _io(action=OUT)), b"boards is NULL"),
    ((BOARDS + 8, 4, 0, _io(action=OUT)), b"misaligned"),
    ((BOARDS, 0, 0, _io(action=OUT)), b"n=0"),
    ((BOARDS, 1 << 32, 0, _io(action=OUT)), b"n=4294967296"),
    ((BOARDS, 4, 0, None), b"io is NULL"),
    ((BOARDS, 4, 0, _io()), b"requests no output"),
    ((BOARDS, 4, 0, _io(value=OUT + 8)), b"mc value needs 16 bytes"),
    ((BOARDS, 4, 0, _io(steps=OUT + 4, action=OUT)), b"mc steps needs 16 bytes"),
    ((BOARDS, 4, 0, _io(rollouts=0, action=OUT)), b"rollouts=0"),
    ((BOARDS, 4, 0, _io(rollouts=65537, value=OUT)), b"rollouts=65537"),
    ((BOARDS, 4, 0, _io(max_steps=0, steps=OUT)), b"max_steps=0"),
    ((BOARDS, 4, 0, _io(max_steps=65536, action=OUT)), b"max_steps=65536"),
    ((BOARDS, 4, (1 << 32) - 3, _io(action=OUT)), b"index_offset=4294967293 n=4"),
])
def test_plain_form_argument_errors(lib, args, message):
    boards, n, index_offset, io = args
    rc = lib.g2048_mc_search_plain(boards, n, index_offset, None if io is None else C.byref(io), None)
    assert rc == -1
    assert message in lib.g2048_last_error()


def test_engine_form_needs_an_engine(lib):
    io = _io(action=OUT)
    assert lib.g2048_mc_search(None, C.byref(io), None) == -1
    assert b"engine is NULL" in lib.g2048_last_error()


def test_python_wrapper_checks_its_input():
    torch = pytest.importorskip("torch")
    import gym2048_amd
    from gym2048_amd import batched
    with pytest.raises(ValueError):
        gym2048_amd.mc_search(torch.zeros((4, 16), dtype=torch.uint8))          # host tensor: refused before the library
    with pytest.raises(ValueError):
        gym2048_amd.mc_search(torch.zeros((4, 15), dtype=torch.uint8))
    assert gym2048_amd.MCSearch._fields == ("action", "value", "steps")
    assert batched.MC_DEFAULT_MAX_STEPS == 65535
    cpu = torch.device("cpu")
    for bad in (dict(rollouts=0), dict(rollouts=65537), dict(rollouts=2.0), dict(rollouts=True), dict(max_steps=0),
                dict(max_steps=65536), dict(seed=-1), dict(seed=1 << 64), dict(index_offset=-1), dict(index_offset=(1 << 32) - 3)):
        kw = dict(rollouts=8, max_steps=10, seed=0, index_offset=0, out=None)
        kw.update(bad)
        with pytest.raises(ValueError, match=next(iter(bad))):
            batched._mc_io(4, cpu, **kw)
    with pytest.raises(ValueError, match="no output"):
        batched._mc_io(4, cpu, 8, 10, 0, 0, gym2048_amd.MCSearch(None, None, None))
    with pytest.raises(ValueError, match="out.value"):
        batched._mc_io(4, cpu, 8, 10, 0, 0, gym2048_amd.MCSearch(None, torch.zeros((4, 4), dtype=torch.int32), None))
    io, out = batched._mc_io(4, cpu, 8, 10, (7 << 32) | 5, (1 << 32) - 4, None)
    assert (io.rollouts, io.max_steps, io.seed) == (8, 10, (7 << 32) | 5)
    assert out.action.shape == (4,) and out.value.shape == out.steps.shape == (4, 4) and out.steps.dtype == torch.int64


def test_record_search_players_and_step_seed():
    from gym2048_amd.transitions import Transitions, mc_step_seed
    seeds = [mc_step_seed(3, t) for t in range(1000)]
    assert len(set(seeds)) == 1000 and 3 not in seeds and all(0 <= s < 1 << 64 for s in seeds)
    assert mc_step_seed((1 << 64) - 1, 5) == ((1 << 64) - 1 + 6 * 0x9E3779B97F4A7C15) % (1 << 64)
    with pytest.raises(ValueError, match="player"):
        Transitions.record_search(None, 1, player="minimax")
