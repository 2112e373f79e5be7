"""CPU: mixed-length n-tuple networks (G2048_NTUPLE_END) at the library's and the Python layer's
doors, without a GPU: the new refusals -- an empty tuple, a cell after an END -- through every entry point of both descriptor
families, the old messages for the old cases, and NTupleNet's flag, shapes, offsets, table(), preset and state_dict."""
import ctypes as C
import os

import pytest

import __graft_entry__ as ge
import ntuple_mixed_ref as mref
from ntuple_helpers import TUPLES_4x6, TUPLES_17x4

BOARDS, OUT, WEIGHTS = 0x10000, 0x20000, 0x30000      # fake device addresses: every call below is refused before they are used
END = 0xff


@pytest.fixture(scope="module")
def lib():
    ge.build_hip()
    from gym2048_amd import _lib
    return _lib.load()


def _fill(net, tuples, L):
    cells = mref.cells_of(tuples, L)
    for t in range(len(tuples)):
        for k in range(6):
            net.cells[t][k] = int(cells[t, k])


def _net(tuples=mref.MIX_ASC, L=4, weights=WEIGHTS, edit=()):
    from gym2048_amd import _lib
    net = _lib.NTupleNetC(len(tuples), L, 10)
    _fill(net, tuples, L)
    for t, k, c in edit:
        net.cells[t][k] = c
    net.weights = weights
    return net


def _staged(S=3, thr=(4, 24), **kw):
    from gym2048_amd import _lib
    net = _lib.NTupleStagedNetC(_net(**kw), S)
    net.thresholds[:len(thr)] = thr
    return net


def _calls(lib, ref_, staged):
    """Every entry point that takes a network of the family, with arguments that are fine but for the network."""
    from gym2048_amd import _lib
    io, sio = _lib.NTupleIO(action=OUT), _lib.NTupleSearchIO(1, OUT, None)
    tc, tr = _lib.NTupleTCC(OUT, OUT), _lib.NTupleTraceC(4, 32768, OUT, OUT)
    f = (lambda name: getattr(lib, "g2048_ntuple_staged_" + name)) if staged else (lambda name: getattr(lib, "g2048_ntuple_" + name))
    calls = [lambda: f("evaluate_plain")(BOARDS, 4, ref_, C.byref(io), None),
             lambda: f("search_plain")(BOARDS, 4, ref_, C.byref(sio), None),
             lambda: f("values_plain")(BOARDS, 4, ref_, OUT, None),
             lambda: f("update_plain")(BOARDS, 4, OUT, 3, ref_, None),
             lambda: f("tc_update_plain")(BOARDS, 4, OUT, 3, 3, ref_, C.byref(tc), None),
             lambda: f("trace_update")(4, OUT, 3, ref_, C.byref(tr), 0, None),
             lambda: f("tc_trace_update")(4, OUT, 3, 3, ref_, C.byref(tc), C.byref(tr), 0, None)]
    if staged:
        calls.append(lambda: lib.g2048_ntuple_stage_plain(BOARDS, 4, ref_, OUT, None))
    return calls


def _engine_calls(lib, ref_, staged):
    """The engine forms: they look at the engine first, so a NULL engine is what they report -- the network check they share
    (one function) is reached through the plain forms above."""
    from gym2048_amd import _lib
    io, sio = _lib.NTupleIO(action=OUT), _lib.NTupleSearchIO(1, OUT, None)
    pre = "g2048_ntuple_staged_" if staged else "g2048_ntuple_"
    return [lambda: getattr(lib, pre + "evaluate")(None, ref_, C.byref(io), None),
            lambda: getattr(lib, pre + "search")(None, ref_, C.byref(sio), None)]


# (edits of the MIX_ASC descriptor at tuple_len 4, message): cells[t] of MIX_ASC are (5,E,E,E) (0,1,E,E) (4,5,6,E) (0,1,4,5)
NEW_ERRORS = [
    ([(0, 0, END)], b"cells[0][0]=G2048_NTUPLE_END: tuple 0 is empty"),
    ([(3, 0, END)], b"cells[3][0]=G2048_NTUPLE_END: tuple 3 is empty"),
    ([(2, 0, END), (2, 1, END), (2, 2, END)], b"cells[2][0]=G2048_NTUPLE_END: tuple 2 is empty"),
    ([(1, 3, 7)], b"cells[1][3]=7: a cell after G2048_NTUPLE_END in tuple 1"),
    ([(0, 2, 5)], b"cells[0][2]=5: a cell after G2048_NTUPLE_END in tuple 0"),
    ([(3, 1, END)], b"cells[3][2]=4: a cell after G2048_NTUPLE_END in tuple 3"),
    ([(0, 3, 16)], b"cells[0][3]=16: a cell after G2048_NTUPLE_END in tuple 0"),
]
OLD_ERRORS = [
    ([(3, 3, 16)], b"cells[3][3]=16: a cell index is 0..15"),
    ([(3, 3, 254)], b"cells[3][3]=254: a cell index is 0..15"),
    ([(2, 1, 0xfe)], b"cells[2][1]=254: a cell index is 0..15"),
    ([(2, 2, 4)], b"cells[2][2]=4: cell repeated within tuple 2"),
    ([(3, 2, 1)], b"cell repeated within tuple 3"),
]


@pytest.mark.parametrize("staged", (False, True), ids=("net", "staged_net"))
@pytest.mark.parametrize("edit, message", NEW_ERRORS + OLD_ERRORS, ids=[m.decode().split(":")[0] + ("" if i < len(NEW_ERRORS) else " old")
                                                                         for i, (_, m) in enumerate(NEW_ERRORS + OLD_ERRORS)])
def test_bad_mixed_descriptor_in_every_entry_point(lib, staged, edit, message):
    net = _staged(edit=edit) if staged else _net(edit=edit)
    calls = _calls(lib, C.byref(net), staged)
    assert len(calls) == (8 if staged else 7)
    for call in calls:
        assert call() == -1
        assert message in lib.g2048_last_error(), lib.g2048_last_error()
    for call in _engine_calls(lib, C.byref(net), staged):
        assert call() == -1 and b"engine is NULL" in lib.g2048_last_error()


@pytest.mark.parametrize("staged", (False, True), ids=("net", "staged_net"))
def test_good_mixed_descriptor_passes_the_network_check(lib, staged):
    """A well-formed mixed descriptor is refused only for what comes after the network check; entries at and beyond
    tuple_len are not read; the old limits keep their messages on a mixed descriptor."""
    make = _staged if staged else _net
    pre = "g2048_ntuple_staged_" if staged else "g2048_ntuple_"
    values = getattr(lib, pre + "values_plain")
    for kw in (dict(), dict(L=6), dict(tuples=mref.MIX_DESC), dict(tuples=mref.MIX_8), dict(tuples=mref.MIX_EXT, L=6),
               dict(tuples=mref.PRESET, L=6), dict(tuples=TUPLES_17x4, L=6), dict(edit=[(0, 4, 3), (1, 5, 200)])):
        net = make(**kw)
        assert values(BOARDS, 4, C.byref(net), None, None) == -1 and b"v is NULL" in lib.g2048_last_error(), kw
    net = make(weights=None)
    assert values(BOARDS, 4, C.byref(net), OUT, None) == -1 and b"net weights is NULL" in lib.g2048_last_error()
    net = make(weights=WEIGHTS + 4)
    assert values(BOARDS, 4, C.byref(net), OUT, None) == -1 and b"ntuple weights need 16 bytes" in lib.g2048_last_error()
    for L, message in ((0, b"tuple_len=0"), (7, b"tuple_len=7")):
        net = make()
        (net.net if staged else net).tuple_len = L
        assert values(BOARDS, 4, C.byref(net), OUT, None) == -1 and message in lib.g2048_last_error()
    if staged:   # the stage does not depend on the tuples: the stage-only call takes a mixed descriptor, weights or not
        net = _staged(weights=None)
        assert lib.g2048_ntuple_stage_plain(BOARDS, 4, C.byref(net), None, None) == -1 and b"stage is NULL" in lib.g2048_last_error()


def test_header_and_abi(lib):
    from gym2048_amd import _lib, ntuple
    text = open(os.path.join(ge.ROOT, "include", "g2048.h")).read()
    assert "#define G2048_NTUPLE_END 0xff\n" in text and ntuple.NTUPLE_END == END == mref.END
    assert "kNtupleEnd = 0xffu" in open(os.path.join(ge.CSRC, "g2048_device.h")).read()
    assert lib.g2048_abi_version() == _lib.ABI_VERSION == 16
    assert C.sizeof(_lib.NTupleNetC) == 72 and C.sizeof(_lib.NTupleStagedNetC) == 96


# ------------------------------------------------------------------------------------------------ Python
def test_the_flag_and_the_shapes():
    torch = pytest.importorskip("torch")
    from gym2048_amd import ntuple
    for bad in ([(0, 1), (2,)], mref.MIX_ASC, [(0, 1, 2, 3, 4, 5), (15,)]):
        with pytest.raises(ValueError, match=r"tuples.*mixed=True"):
            ntuple.NTupleNet(bad, device="cpu")
    for bad in ([(0, 1), ()], [(0, 1), range(7)], [(0, 1), (3, 3)], [(0, 1), (16,)]):
        with pytest.raises(ValueError, match="tuples"):
            ntuple.NTupleNet(bad, device="cpu", mixed=True)
    net = ntuple.NTupleNet(mref.MIX_ASC, frac_bits=12, device="cpu", mixed=True)
    assert net.mixed and net.tuples == mref.MIX_ASC and net.n_tuples == 4 and net.tuple_len == 4
    assert net.tuple_lens == (1, 2, 3, 4) and net.table_offsets == (0, 16, 272, 4368) and net.n_weights == 69904
    assert net.weights.dtype == torch.int32 and tuple(net.weights.shape) == (69904,) and not net.weights.any()
    assert (net._c.n_tuples, net._c.tuple_len, net._c.frac_bits, net._c.weights) == (4, 4, 12, net.weights.data_ptr())
    assert [[net._c.cells[t][k] for k in range(4)] for t in range(4)] == mref.cells_of(mref.MIX_ASC)[:4, :4].tolist()
    assert [net._c.cells[0][k] for k in range(4)] == [5, END, END, END]
    assert net._fn("values_plain").__name__ == "g2048_ntuple_values_plain"
    # table(): a view of one table
    for t in range(4):
        tab = net.table(t)
        assert tuple(tab.shape) == (16 ** (t + 1),) and tab.data_ptr() == net.weights.data_ptr() + 4 * net.table_offsets[t]
    net.table(2)[5] = -9
    assert net.weights[272 + 5] == -9 and int(net.weights.count_nonzero()) == 1
    for bad in (lambda: net.table(4), lambda: net.table(-1), lambda: net.table(0, stage=0)):
        with pytest.raises(ValueError, match="t must|stage"):
            bad()
    # staged: [S, W]
    st = ntuple.NTupleNet(mref.MIX_DESC, device="cpu", mixed=True, stages=(4, 24))
    assert tuple(st.weights.shape) == (3, 69904) and st.table_offsets == (0, 65536, 65536 + 4096, 65536 + 4096 + 256)
    assert st._fn("values_plain").__name__ == "g2048_ntuple_staged_values_plain" and st._c.net.tuple_len == 4
    assert [st._c.net.cells[3][k] for k in range(4)] == [5, END, END, END]
    assert st.table(3, stage=2).data_ptr() == st.weights.data_ptr() + 4 * (2 * 69904 + st.table_offsets[3])
    with pytest.raises(ValueError, match="stage"):
        st.table(0)
    tc = ntuple.NTupleTC(st)
    assert tc.err.shape == tc.mag.shape == st.weights.shape and "mixed" in ntuple.NTupleTC.__doc__
    st.weights[0, 7], tc.err[1, 7] = 3, 5
    st.promote(0, 1, tc)
    assert st.weights[1, 7] == 3 and not tc.err[1].any()
    # with equal lengths the flag changes nothing; a uniform net has the new attributes and table() too
    for flag in (False, True):
        uni = ntuple.NTupleNet(TUPLES_17x4, device="cpu", mixed=flag)
        assert not uni.mixed and tuple(uni.weights.shape) == (5, 16 ** 4) and uni.tuple_lens == (4,) * 5 and uni.n_weights == 5 * 16 ** 4
        assert uni.table_offsets == tuple(t * 16 ** 4 for t in range(5)) and uni.table(3).data_ptr() == uni.weights[3].data_ptr()
        assert [uni._c.cells[4][k] for k in range(6)] == [5, 6, 9, 10, 0, 0]


def test_the_preset_is_redundant():
    pytest.importorskip("torch")
    from gym2048_amd import ntuple
    preset = ntuple.TUPLES["4x6+4x4"]
    assert preset == mref.PRESET and preset[:4] == ntuple.TUPLES["4x6"] == TUPLES_4x6
    assert preset[4:] == ((0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 4, 5), (5, 6, 9, 10))
    for small in preset[4:]:                       # each 4-tuple is a sub-shape of one of the 6-tuples
        assert any(set(small) <= set(big) for big in preset[:4]), small
    net = ntuple.NTupleNet("4x6+4x4", device="cpu")        # a ragged name needs no flag
    assert net.mixed and net.n_weights == 4 * 16 ** 6 + 4 * 16 ** 4 == 67371008 and tuple(net.weights.shape) == (67371008,)
    assert net.tuple_len == 6 and net.tuple_lens == (6, 6, 6, 6, 4, 4, 4, 4) and net.table_offsets[4] == 4 * 16 ** 6
    assert [net._c.cells[4][k] for k in range(6)] == [0, 1, 2, 3, END, END]


def test_state_dict_round_trip_and_refusals():
    torch = pytest.importorskip("torch")
    from gym2048_amd import ntuple
    net = ntuple.NTupleNet(mref.MIX_ASC, device="cpu", mixed=True)
    net.weights[4368 + 9] = -5
    state = net.state_dict()
    assert state["tuples"] == mref.MIX_ASC and tuple(state["weights"].shape) == (69904,)
    other = ntuple.NTupleNet([list(t) for t in mref.MIX_ASC], device="cpu", mixed=True)
    ptr = other.weights.data_ptr()
    other.load_state_dict(state)
    assert other.weights[4368 + 9] == -5 and other.weights.data_ptr() == ptr and torch.equal(other.weights, net.weights)
    desc = ntuple.NTupleNet(mref.MIX_DESC, device="cpu", mixed=True)                  # the same W, other tuples
    uniform = ntuple.NTupleNet(tuple(t[:1] for t in mref.MIX_ASC), device="cpu")
    for wrong in (desc, uniform):
        with pytest.raises(ValueError, match="other tuples"):
            wrong.load_state_dict(state)
        with pytest.raises(ValueError, match="other tuples"):
            net.load_state_dict(wrong.state_dict())
    staged = ntuple.NTupleNet(mref.MIX_ASC, device="cpu", mixed=True, stages=(4,))
    with pytest.raises(ValueError, match="stages"):
        staged.load_state_dict(state)
    state["weights"] = state["weights"].reshape(1, -1)
    with pytest.raises(ValueError, match="weights must be int32"):
        net.load_state_dict(state)
