"""CPU: the n-tuple network entry points (g2048_ntuple_evaluate, _evaluate_plain, _values_plain, _update_plain) are
exported, bound with pinned struct layouts, refuse bad arguments with a message before touching a device, and leave the ABI
version at 16 -- so these checks run without a GPU.  The Python layer refuses bad input before the library."""
import ctypes as C
import os

import pytest

import __graft_entry__ as ge
import ntuple_ref as ref
from ntuple_helpers import TUPLES_4x6, TUPLES_17x4

NAMES = ("g2048_ntuple_evaluate", "g2048_ntuple_evaluate_plain", "g2048_ntuple_values_plain", "g2048_ntuple_update_plain")


@pytest.fixture(scope="module")
def lib():
    ge.build_hip()
    from gym2048_amd import _lib
    return _lib.load()


# fake device addresses: every case below is refused before the pointer could be used
BOARDS, OUT, WEIGHTS = 0x10000, 0x20000, 0x30000


def _net(T=5, L=4, F=10, tuples=TUPLES_17x4, weights=WEIGHTS):
    from gym2048_amd import _lib
    net = _lib.NTupleNetC(T, L, F)
    for t, cells in enumerate(tuples):
        for k, c in enumerate(cells):
            net.cells[t][k] = c
    net.weights = weights
    return net


def _io(**kw):
    from gym2048_amd import _lib
    return _lib.NTupleIO(**kw)


def test_symbols_exported_and_abi_still_16(lib):
    from gym2048_amd import _lib
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.g2048_abi_version() == _lib.ABI_VERSION == 16


def test_struct_layouts():
    from gym2048_amd import _lib
    N, IO = _lib.NTupleNetC, _lib.NTupleIO
    assert C.sizeof(N) == 72          # three uint32, 48 cell bytes, padding to 8, a pointer
    assert (N.n_tuples.offset, N.tuple_len.offset, N.frac_bits.offset, N.cells.offset, N.weights.offset) == (0, 4, 8, 12, 64)
    assert C.sizeof(IO) == 40 and [f[0] for f in IO._fields_] == ["value", "action", "best", "after", "after_value"]


def test_header_pins_the_limits():
    text = open(os.path.join(ge.ROOT, "include", "g2048.h")).read()
    for line in ("#define G2048_NTUPLE_MAX_TUPLES 8\n", "#define G2048_NTUPLE_MAX_LEN 6\n", "#define G2048_NTUPLE_ILLEGAL INT64_MIN\n",
                 "#define G2048_NTUPLE_MAX_FRAC_BITS 16\n", "#define G2048_NTUPLE_MAX_LR_SHIFT 40\n"):
        assert line in text, line
    dev = open(os.path.join(ge.CSRC, "g2048_device.h")).read()
    assert "kNtupleMaxTuples = 8, kNtupleMaxLen = 6, kNtupleMaxFrac = 16, kNtupleMaxShift = 40" in dev


def _bad_cells(which):
    net = _net()
    if which == "range":
        net.cells[2][3] = 16
    else:
        net.cells[4][1] = net.cells[4][3]
    return net


NET_ERRORS = [
    (lambda: None, b"net is NULL"),
    (lambda: _net(T=0), b"n_tuples=0"),
    (lambda: _net(T=9), b"n_tuples=9"),
    (lambda: _net(L=0), b"tuple_len=0"),
    (lambda: _net(L=7), b"tuple_len=7"),
    (lambda: _net(F=17), b"frac_bits=17"),
    (lambda: _bad_cells("range"), b"cells[2][3]=16"),
    (lambda: _bad_cells("repeat"), b"cell repeated within tuple 4"),
    (lambda: _net(weights=None), b"net weights is NULL"),
    (lambda: _net(weights=WEIGHTS + 4), b"ntuple weights need 16 bytes"),
]


@pytest.mark.parametrize("make, message", NET_ERRORS, ids=[m.decode() for _, m in NET_ERRORS])
def test_network_errors_in_every_entry_point(lib, make, message):
    net = make()
    ref_ = None if net is None else C.byref(net)
    io = _io(action=OUT)
    calls = (lambda: lib.g2048_ntuple_evaluate_plain(BOARDS, 4, ref_, C.byref(io), None),
             lambda: lib.g2048_ntuple_values_plain(BOARDS, 4, ref_, OUT, None),
             lambda: lib.g2048_ntuple_update_plain(BOARDS, 4, OUT, 3, ref_, None))
    for call in calls:
        assert call() == -1
        assert message in lib.g2048_last_error()


@pytest.mark.parametrize("boards, n, message", [(None, 4, b"boards is NULL"), (BOARDS + 8, 4, b"misaligned"), (BOARDS, 0, b"n=0"),
                                                (BOARDS, 1 << 32, b"n=4294967296"), (BOARDS, (1 << 32) - 255, b"n=4294967041")])
def test_board_errors_in_every_plain_entry_point(lib, boards, n, message):
    net, io = _net(), _io(action=OUT)
    for rc in (lib.g2048_ntuple_evaluate_plain(boards, n, C.byref(net), C.byref(io), None),
               lib.g2048_ntuple_values_plain(boards, n, C.byref(net), OUT, None),
               lib.g2048_ntuple_update_plain(boards, n, OUT, 3, C.byref(net), None)):
        assert rc == -1 and message in lib.g2048_last_error()


@pytest.mark.parametrize("io, message", [
    (None, b"io is NULL"),
    (_io, b"requests no output"),
    (lambda: _io(value=OUT + 8), b"ntuple value needs 16 bytes"),
    (lambda: _io(after=OUT + 4, action=OUT), b"ntuple after needs 16 bytes"),
    (lambda: _io(best=OUT + 4), b"best and after_value need 8 bytes"),
    (lambda: _io(after_value=OUT + 2), b"best and after_value need 8 bytes"),
])
def test_evaluate_output_errors(lib, io, message):
    net = _net()
    io = None if io is None else io()
    assert lib.g2048_ntuple_evaluate_plain(BOARDS, 4, C.byref(net), None if io is None else C.byref(io), None) == -1
    assert message in lib.g2048_last_error()


def test_values_update_and_engine_form_errors(lib):
    net, io = _net(), _io(action=OUT)
    assert lib.g2048_ntuple_values_plain(BOARDS, 4, C.byref(net), None, None) == -1 and b"v is NULL" in lib.g2048_last_error()
    assert lib.g2048_ntuple_values_plain(BOARDS, 4, C.byref(net), OUT + 4, None) == -1 and b"v needs 8 bytes" in lib.g2048_last_error()
    assert lib.g2048_ntuple_update_plain(BOARDS, 4, None, 3, C.byref(net), None) == -1 and b"delta is NULL" in lib.g2048_last_error()
    assert lib.g2048_ntuple_update_plain(BOARDS, 4, OUT + 4, 3, C.byref(net), None) == -1 and b"delta needs 8 bytes" in lib.g2048_last_error()
    assert lib.g2048_ntuple_update_plain(BOARDS, 4, OUT, 41, C.byref(net), None) == -1 and b"lr_shift=41" in lib.g2048_last_error()
    assert lib.g2048_ntuple_evaluate(None, C.byref(net), C.byref(io), None) == -1 and b"engine is NULL" in lib.g2048_last_error()


def test_default_shapes_are_data():
    """The package's named shapes are the ones the tests use; the five 4-tuples of "17x4" cover, by their symmetric images,
    exactly the 4 rows, 4 columns and 9 2x2 squares."""
    pytest.importorskip("torch")
    from gym2048_amd.ntuple import TUPLES
    assert TUPLES["4x6"] == TUPLES_4x6 and TUPLES["17x4"] == TUPLES_17x4
    cells = tuple(range(16))
    placed = {frozenset(s[c] for c in t) for s in ref.symmetries(cells) for t in TUPLES["17x4"]}
    rows = {frozenset(range(4 * r, 4 * r + 4)) for r in range(4)}
    cols = {frozenset(range(c, 16, 4)) for c in range(4)}
    squares = {frozenset((4 * r + c, 4 * r + c + 1, 4 * r + c + 4, 4 * r + c + 5)) for r in range(3) for c in range(3)}
    assert placed == rows | cols | squares and len(placed) == 17


def test_python_layer_checks_its_input():
    torch = pytest.importorskip("torch")
    import gym2048_amd
    from gym2048_amd import batched, ntuple
    assert gym2048_amd.NTupleNet is batched.NTupleNet is ntuple.NTupleNet and batched.td_step is ntuple.td_step
    assert gym2048_amd.NTupleEval._fields == ("value", "action", "best", "after", "after_value")
    for bad in (dict(tuples="5x5"), dict(tuples=()), dict(tuples=[(0,)] * 9), dict(tuples=[(0, 1), (2,)]), dict(tuples=[range(7)]),
                dict(tuples=[(0, 16)]), dict(tuples=[(3, 3)]), dict(tuples=[(0, 1.5)]), dict(tuples=5), dict(frac_bits=-1),
                dict(frac_bits=17), dict(frac_bits=1.0)):
        with pytest.raises(ValueError, match="tuples" if "tuples" in bad else "frac_bits"):
            ntuple.NTupleNet(device="cpu", **bad)
    net = ntuple.NTupleNet("17x4", frac_bits=12, device="cpu")
    assert net.weights.dtype == torch.int32 and tuple(net.weights.shape) == (5, 16 ** 4) and not net.weights.any()
    assert (net.n_tuples, net.tuple_len, net.frac_bits) == (5, 4, 12)
    assert (net._c.n_tuples, net._c.tuple_len, net._c.frac_bits, net._c.weights) == (5, 4, 12, net.weights.data_ptr())
    assert [net._c.cells[3][k] for k in range(4)] == [1, 2, 5, 6]
    assert tuple(ntuple.NTupleNet(device="cpu").weights.shape) == (4, 16 ** 6)
    host = torch.zeros((4, 16), dtype=torch.uint8)
    for call in (lambda: net.values(host), lambda: net.evaluate(host), lambda: net.update(host, torch.zeros(4, dtype=torch.int64), 3),
                 lambda: net.values(torch.zeros((4, 15), dtype=torch.uint8)), lambda: net.values(host.to(torch.int32))):
        with pytest.raises(ValueError, match="boards"):    # host tensors, wrong shape, wrong dtype: refused before the library
            call()
    cpu = torch.device("cpu")
    with pytest.raises(ValueError, match="no output"):
        ntuple._eval_io(4, cpu, ntuple.NTupleEval(None, None, None, None, None))
    with pytest.raises(ValueError, match="out.value"):
        ntuple._eval_io(4, cpu, ntuple.NTupleEval(torch.zeros((4, 4), dtype=torch.int32), None, None, None, None))
    with pytest.raises(ValueError, match="out.after"):
        ntuple._eval_io(4, cpu, ntuple.NTupleEval(None, None, None, torch.zeros((4, 4, 4), dtype=torch.uint8), None))
    io, out = ntuple._eval_io(4, cpu, None)
    assert out.value.shape == (4, 4) and out.after.shape == (4, 16) and out.best.dtype == torch.int64 and io.after == out.after.data_ptr()
    with pytest.raises(ValueError, match="weights are on"):
        net._ref(torch.device("cuda", 0))
    # state_dict round trip; a state of another shape is refused
    net.weights[2, 77] = -5
    other = ntuple.NTupleNet("17x4", frac_bits=12, device="cpu")
    ptr = other.weights.data_ptr()
    other.load_state_dict(net.state_dict())
    assert other.weights[2, 77] == -5 and other.weights.data_ptr() == ptr
    with pytest.raises(ValueError, match="other tuples"):
        ntuple.NTupleNet("17x4", frac_bits=10, device="cpu").load_state_dict(net.state_dict())


def test_record_search_names_the_old_players_first():
    pytest.importorskip("torch")
    from gym2048_amd.transitions import Transitions
    with pytest.raises(ValueError, match="player must be 'expectimax', 'mc' or 'ntuple'"):
        Transitions.record_search(None, 1, player="minimax")
    with pytest.raises(ValueError, match="needs net"):
        Transitions.record_search(None, 1, player="ntuple")
