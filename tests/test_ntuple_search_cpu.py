"""CPU: the n-tuple expectimax entry points (g2048_ntuple_search, g2048_ntuple_search_plain) are exported, bound with a
pinned struct layout, refuse bad arguments with a message before touching a device, and leave the ABI version at 16 -- so
these checks run without a GPU.  The Python layer refuses bad input before the library."""
import ctypes as C
import os

import pytest

import __graft_entry__ as ge
from ntuple_helpers import TUPLES_17x4

NAMES = ("g2048_ntuple_search", "g2048_ntuple_search_plain")


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


def _io(depth=1, **kw):
    from gym2048_amd import _lib
    return _lib.NTupleSearchIO(depth, **kw)


def test_symbols_exported_and_abi_still_16(lib):
    from gym2048_amd import _lib
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.g2048_abi_version() == _lib.ABI_VERSION == 16


def test_struct_layout():
    from gym2048_amd import _lib
    IO = _lib.NTupleSearchIO
    assert C.sizeof(IO) == 24          # a uint32 padded to 8, two pointers
    assert (IO.depth.offset, IO.action.offset, IO.value.offset) == (0, 8, 16)
    assert [f[0] for f in IO._fields_] == ["depth", "action", "value"]


def test_header_pins_the_depth_limit():
    text = open(os.path.join(ge.ROOT, "include", "g2048.h")).read()
    assert "#define G2048_NTUPLE_SEARCH_MAX_DEPTH 2\n" in text
    dev = open(os.path.join(ge.CSRC, "g2048_device.h")).read()
    assert "kNtupleSearchMaxDepth = 2;" in dev
    pytest.importorskip("torch")
    from gym2048_amd import ntuple
    assert ntuple.SEARCH_MAX_DEPTH == 2


def _bad_cells(which):
    net = _net()
    if which == "range":
        net.cells[2][3] = 16
    else:
        net.cells[4][1] = net.cells[4][3]
    return net


# the network checks of g2048_ntuple_evaluate, reused
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
def test_network_errors(lib, make, message):
    net = make()
    io = _io(action=OUT)
    assert lib.g2048_ntuple_search_plain(BOARDS, 4, None if net is None else C.byref(net), C.byref(io), None) == -1
    assert message in lib.g2048_last_error()


@pytest.mark.parametrize("boards, n, message", [(None, 4, b"boards is NULL"), (BOARDS + 8, 4, b"misaligned buffer: boards"), (BOARDS, 0, b"n=0"),
                                                (BOARDS, 1 << 32, b"n=4294967296"), (BOARDS, (1 << 32) - 255, b"n=4294967041")])
def test_board_errors(lib, boards, n, message):
    net, io = _net(), _io(action=OUT)
    assert lib.g2048_ntuple_search_plain(boards, n, C.byref(net), C.byref(io), None) == -1
    assert message in lib.g2048_last_error()


@pytest.mark.parametrize("io, message", [
    (None, b"io is NULL"),
    (_io, b"g2048_ntuple_search_io requests no output"),
    (lambda: _io(value=OUT + 8), b"ntuple search value needs 16 bytes"),
    (lambda: _io(depth=0, action=OUT), b"depth=0: need 1 <= depth <= 2"),
    (lambda: _io(depth=3, action=OUT), b"depth=3: need 1 <= depth <= 2"),
])
def test_output_and_depth_errors(lib, io, message):
    net = _net()
    io = None if io is None else io()
    assert lib.g2048_ntuple_search_plain(BOARDS, 4, C.byref(net), None if io is None else C.byref(io), None) == -1
    assert message in lib.g2048_last_error()


def test_engine_form_errors(lib):
    net, io = _net(), _io(action=OUT)
    assert lib.g2048_ntuple_search(None, C.byref(net), C.byref(io), None) == -1 and b"engine is NULL" in lib.g2048_last_error()


def test_python_layer_checks_its_input():
    torch = pytest.importorskip("torch")
    import gym2048_amd
    from gym2048_amd import batched, ntuple
    assert gym2048_amd.NTupleSearch is batched.NTupleSearch is ntuple.NTupleSearch
    assert gym2048_amd.NTupleSearch._fields == ("action", "value")
    net = ntuple.NTupleNet("17x4", frac_bits=12, device="cpu")
    host = torch.zeros((4, 16), dtype=torch.uint8)
    for call in (lambda: net.search(host), lambda: net.search(torch.zeros((4, 15), dtype=torch.uint8)), lambda: net.search(host.to(torch.int32))):
        with pytest.raises(ValueError, match="boards"):    # host tensors, wrong shape, wrong dtype: refused before the library
            call()
    cpu = torch.device("cpu")
    for depth in (0, 3, -1, 1.0, True, None):
        with pytest.raises(ValueError, match="depth"):
            ntuple._search_io(4, cpu, depth, None)
    with pytest.raises(ValueError, match="no output"):
        ntuple._search_io(4, cpu, 1, ntuple.NTupleSearch(None, None))
    with pytest.raises(ValueError, match="out.value"):
        ntuple._search_io(4, cpu, 1, ntuple.NTupleSearch(None, torch.zeros((4, 4), dtype=torch.int32)))
    with pytest.raises(ValueError, match="out.action"):
        ntuple._search_io(4, cpu, 1, ntuple.NTupleSearch(torch.zeros(5, dtype=torch.uint8), None))
    io, out = ntuple._search_io(4, cpu, 2, None)
    assert io.depth == 2 and out.action.shape == (4,) and out.value.shape == (4, 4) and out.value.dtype == torch.int64
    assert io.action == out.action.data_ptr() and io.value == out.value.data_ptr()
    io, out = ntuple._search_io(4, cpu, 1, ntuple.NTupleSearch(torch.zeros(4, dtype=torch.uint8), None))
    assert not io.value and out.value is None


def test_record_search_refuses_a_net_depth_out_of_range():
    pytest.importorskip("torch")
    from gym2048_amd import ntuple
    from gym2048_amd.transitions import Transitions
    net = ntuple.NTupleNet("17x4", device="cpu")
    for bad in (3, -1, 1.5):
        with pytest.raises(ValueError, match="net_depth"):
            Transitions.record_search(None, 1, player="ntuple", net=net, net_depth=bad)
    with pytest.raises(ValueError, match="needs net"):
        Transitions.record_search(None, 1, player="ntuple", net_depth=1)
