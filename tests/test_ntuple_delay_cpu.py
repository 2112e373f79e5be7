"""CPU: the n-tuple delay (include/g2048.h "N-tuple delay") without a device.  The reference
tests/ntuple_delay_ref.py holds the definition twice -- a ring model and the closed form of consequence 1 -- and the first tests
show that the two agree, that every pushed afterstate is applied exactly once, and consequence 3 against tests/ntuple_ref.py.
Then push over every len byte and the clamps; then the doors: the new symbols, their signatures, the argument checks of the C
ABI (before any HIP call) and of the Python classes."""
import ctypes as C
import os

import numpy as np
import pytest

import __graft_entry__ as ge
import ntuple_delay_ref as dref
import ntuple_ref as ref
import ntuple_tc_ref as tcref
import ntuple_trace_ref as tref
from analysis_helpers import mixed_boards
from ntuple_helpers import TUPLES_17x4

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
MAXD = 1 << 40
LAMS = (0, 1, 32768, 65535, 65536)
NAMES = ("g2048_ntuple_delay_push", "g2048_ntuple_delay_update", "g2048_ntuple_tc_delay_update",
         "g2048_ntuple_staged_delay_update", "g2048_ntuple_staged_tc_delay_update")


def _sequence(pushes, seed):
    """deltas[t][i], terms[t][i] for 8 boards: board 0 never ends, board 1 ends at every push from 10 to 14 (consecutive
    ends) and at the last, board 2 ends at the last push only, the others at random (p = 1/4); deltas mix small values whose
    decayed parts floor to 0 or -1, large ones, the clamp's edges and the int64 extremes."""
    rng = np.random.default_rng(seed)
    n = 8
    special = [1, -1, 3, -3, MAXD, -MAXD, MAXD + 1, -MAXD - 1, INT64_MAX, INT64_MIN, 0]
    deltas, terms = [], []
    for t in range(pushes):
        d = [int(x) << int(s) for x, s in zip(rng.integers(-(1 << 20), 1 << 20, n), rng.integers(0, 22, n))]
        d[(t * 3) % n] = special[t % len(special)]
        term = [bool(x) for x in rng.integers(0, 4, n) == 0]
        term[0] = False
        term[1] = 10 <= t <= 14 or t == pushes - 1
        term[2] = t == pushes - 1
        deltas.append(d)
        terms.append(term)
    return deltas, terms


@pytest.mark.parametrize("H", range(1, 9))
def test_ring_model_equals_closed_form_and_applies_exactly_once(H):
    deltas, terms = _sequence(40, 100 + H)
    assert not any(t[0] for t in terms) and all(terms[t][1] for t in range(10, 15)) and any(t[3] for t in terms)
    for lam in LAMS:
        want = dref.closed_totals(deltas, terms, H, lam)
        got = dref.applied_totals(deltas, terms, H, lam)
        assert set(got) == set(want) and len(want) == 40 * 8            # every pushed afterstate is applied ...
        assert all(len(v) == 1 for v in got.values())                   # ... exactly once ...
        assert {k: v[0] for k, v in got.items()} == want                # ... with the closed form's total
        assert all(abs(v) <= 8 * MAXD for v in want.values())
    # without the FLUSH exactly the afterstates of the last H - 1 pushes of boards still running are missing
    got = dref.applied_totals(deltas, terms, H, 32768, flush=False)
    missing = set(want) - set(got)
    last_end = {i: max([t for t in range(40) if terms[t][i]], default=-1) for i in range(8)}
    assert missing == {(t, i) for i in range(8) for t in range(max(40 - (H - 1), last_end[i] + 1), 40)}


def test_totals_differ_from_one_step_when_lambda_is_not_zero():
    deltas, terms = _sequence(12, 7)
    one = dref.closed_totals(deltas, terms, 1, 32768)
    assert one == {(t, i): tcref.clamp_delta(deltas[t][i]) for t in range(12) for i in range(8)}
    assert dref.closed_totals(deltas, terms, 4, 0) == one               # lambda = 0: p_k = 0 for k > 0
    assert dref.closed_totals(deltas, terms, 4, 32768) != one


@pytest.mark.parametrize("H", (1, 3, 8))
def test_lambda_0_td_equals_the_plain_updates_after_the_flush(H):
    """Consequence 3, against ntuple_ref: integer adds commute."""
    n, pushes = 6, 11
    rng = np.random.default_rng(31 + H)
    boards = mixed_boards(n * pushes, 32).reshape(pushes, n, 16)
    net = ref.Net(TUPLES_17x4)
    net.weights[:] = rng.integers(-(1 << 31), 1 << 31, net.weights.shape)
    want, got, dl = net.copy(), net.copy(), dref.Delay(n, H, 0)
    applied = 0
    for t in range(pushes):
        av, best = rng.integers(-(1 << 36), 1 << 36, n), rng.integers(-(1 << 36), 1 << 36, n)
        term = rng.integers(0, 3, n) == 0
        delta = dref.push(dl, boards[t], av, best, term)
        assert (np.abs(delta) <= MAXD).all()
        ref.update(want, boards[t], delta, 5)
        applied += len(dref.due_items(dl, dref.STEP)[1])
        dref.delay_update(got, dl, 5)
    assert H == 1 or (got.weights != want.weights).any()               # errors are still pending
    applied += len(dref.due_items(dl, dref.FLUSH)[1])
    dref.delay_update(got, dl, 5, dref.FLUSH)
    assert applied == n * pushes and np.array_equal(got.weights, want.weights) and (want.weights != net.weights).any()


@pytest.mark.parametrize("H", range(1, 9))
def test_push_is_total_over_every_len_byte(H):
    """Every old byte 0..255, both flags, the garbage bytes 0x7f and 0xff among them: the len byte is the trace push's, the
    slot's accumulator is overwritten with d, exactly the L - 1 older valid slots collect, and nothing else moves."""
    old = np.arange(256, dtype=np.uint8)
    for term in (0, 1):
        dl = dref.Delay(256, H, 65536)
        dl.len[:] = old
        dl.slot = (H + 1) % H                                           # some slot in the middle of the ring
        for s in range(H):
            dl.acc[s] = [1000 * (s + 1) + i for i in range(256)]
        before = dl.copy()
        delta = dref.push(dl, np.zeros((256, 16), np.uint8), np.full(256, -77), np.zeros(256, np.int64), np.full(256, term))
        assert (delta == 77).all() and dl.slot == (before.slot + 1) % H
        for b in (0, 1, H, H + 1, 0x7f, 0x80, 0x80 | H, 0xff) + tuple(range(256)):
            l = 0 if b & 0x80 else min(b & 0x7f, H)
            L = min(l + 1, H)
            assert int(dl.len[b]) == (L | (0x80 if term else 0)) == tref.push_len(b, H, bool(term))
            assert dl.acc[dl.slot][b] == 77
            for k in range(1, H):
                s = (dl.slot + H - k) % H
                assert dl.acc[s][b] == before.acc[s][b] + (77 if k < L else 0), (H, b, k)


def test_clamps_of_delta_and_of_the_accumulator():
    special = [MAXD, -MAXD, MAXD + 1, -MAXD - 1, INT64_MAX, INT64_MIN]
    dl = dref.Delay(6, 8, 65536)
    z = np.zeros((6, 16), np.uint8)
    delta = dref.push(dl, z, np.zeros(6, np.int64), np.array(special, np.int64), np.zeros(6, np.uint8))
    assert delta.tolist() == special                                    # delta itself is not clamped ...
    assert dl.acc[0] == [MAXD, -MAXD, MAXD, -MAXD, MAXD, -MAXD]         # ... what the accumulators collect is
    for _ in range(7):
        dref.push(dl, z, np.zeros(6, np.int64), np.array(special, np.int64), np.zeros(6, np.uint8))
    assert dl.slot == 7 and dl.acc[0] == [8 * MAXD, -8 * MAXD] * 3      # eight pushes of +-2^40 at lambda = 1: +-2^43
    assert [dl.acc[s][0] for s in range(8)] == [(8 - s) * MAXD for s in range(8)]
    boards, Ds = dref.due_items(dl, dref.STEP)
    assert len(Ds) == 6 and Ds == [MAXD, -MAXD] * 3                     # only k = 7 is due, and D clamps
    boards, Ds = dref.due_items(dl, dref.FLUSH)
    assert len(Ds) == 42 and set(Ds) == {MAXD, -MAXD}


# ------------------------------------------------------------------------------------------------ the doors
AFTER, VALUE, BEST, TERM, DELTA, WEIGHTS, HIST, LEN, ERR, MAG, ACC = (0x10000 * k for k in range(1, 12))


@pytest.fixture(scope="module")
def lib():
    ge.build_hip()
    from gym2048_amd import _lib
    return _lib.load()


def _net(T=5, weights=WEIGHTS, staged=False):
    from gym2048_amd import _lib
    net = _lib.NTupleNetC(T, 4, 10)
    for t, cells in enumerate(TUPLES_17x4):
        for k, c in enumerate(cells):
            net.cells[t][k] = c
    net.weights = weights
    if staged:
        st = _lib.NTupleStagedNetC(net, 2)
        st.thresholds[0] = 16
        return C.byref(st)
    return C.byref(net)


def _dl(depth=4, lam=32768, hist=HIST, ln=LEN, acc=ACC):
    from gym2048_amd import _lib
    return C.byref(_lib.NTupleDelayC(depth, lam, hist, ln, acc))


def _tc(err=ERR, mag=MAG):
    from gym2048_amd import _lib
    return C.byref(_lib.NTupleTCC(err, mag))


def test_symbols_signatures_struct_and_header(lib):
    from gym2048_amd import _lib
    u64, u32, P = C.c_uint64, C.c_uint32, C.c_void_p
    N, S, T, D = (C.POINTER(c) for c in (_lib.NTupleNetC, _lib.NTupleStagedNetC, _lib.NTupleTCC, _lib.NTupleDelayC))
    want = {NAMES[0]: [P, P, P, P, u64, D, u32, P, P], NAMES[1]: [u64, u32, u32, N, D, u32, P],
            NAMES[2]: [u64, u32, u32, u32, N, T, D, u32, P], NAMES[3]: [u64, u32, u32, S, D, u32, P],
            NAMES[4]: [u64, u32, u32, u32, S, T, D, u32, P]}
    for name in NAMES:
        assert hasattr(lib, name) and _lib.SIGNATURES[name] == (C.c_int, want[name])
    assert lib.g2048_abi_version() == _lib.ABI_VERSION == 16
    X = _lib.NTupleDelayC
    assert C.sizeof(X) == 32 and (X.depth.offset, X.lambda_.offset, X.hist.offset, X.len.offset, X.acc.offset) == (0, 4, 8, 16, 24)
    header = open(os.path.join(ge.ROOT, "include", "g2048.h")).read()
    assert "#define G2048_NTUPLE_DELAY_STEP  0u\n" in header and "#define G2048_NTUPLE_DELAY_FLUSH 1u\n" in header
    assert all(f"int {name}(" in header for name in NAMES)
    from gym2048_amd import ntuple
    assert (ntuple.DELAY_STEP, ntuple.DELAY_FLUSH) == (0, 1) == (dref.STEP, dref.FLUSH)


def _all_calls(lib, dl, slot, n=4, shift=3, mode=0, phases=3, net=_net, tc=_tc):
    plain, staged = (None, None) if net is None else (net(), net(staged=True))
    t = None if tc is None else tc()
    return (lib.g2048_ntuple_delay_push(AFTER, VALUE, BEST, TERM, n, dl, slot, DELTA, None),
            lib.g2048_ntuple_delay_update(n, shift, mode, plain, dl, slot, None),
            lib.g2048_ntuple_staged_delay_update(n, shift, mode, staged, dl, slot, None),
            lib.g2048_ntuple_tc_delay_update(n, shift, phases, mode, plain, t, dl, slot, None),
            lib.g2048_ntuple_staged_tc_delay_update(n, shift, phases, mode, staged, t, dl, slot, None))


DELAY_ERRORS = [
    (None, 0, b"dl is NULL"),
    (dict(hist=None), 0, b"delay hist is NULL"),
    (dict(ln=None), 0, b"delay len is NULL"),
    (dict(acc=None), 0, b"delay acc is NULL"),
    (dict(depth=0), 0, b"depth=0"),
    (dict(depth=9), 0, b"depth=9"),
    (dict(lam=65537), 0, b"lambda=65537"),
    (dict(), 4, b"slot=4"),
    (dict(depth=1), 1, b"slot=1"),
    (dict(hist=HIST + 8), 0, b"delay hist needs 16 bytes"),
    (dict(acc=ACC + 4), 0, b"delay acc needs 8 bytes"),
]


@pytest.mark.parametrize("kw, slot, message", DELAY_ERRORS, ids=[m.decode() for _, _, m in DELAY_ERRORS])
def test_delay_errors_in_every_entry_point(lib, kw, slot, message):
    dl = None if kw is None else _dl(**kw)
    for k in range(5):
        assert _all_calls(lib, dl, slot)[k] == -1 and message in lib.g2048_last_error()


PUSH_ERRORS = [
    (dict(after=None), b"after is NULL"), (dict(value=None), b"after_value is NULL"), (dict(best=None), b"best_next is NULL"),
    (dict(term=None), b"terminated is NULL"), (dict(delta=None), b"delta is NULL"),
    (dict(n=0), b"n=0"), (dict(n=1 << 32), b"n=4294967296"),
    (dict(after=AFTER + 8), b"delay after needs 16 bytes"),
    (dict(value=VALUE + 4), b"after_value, best_next and delta need 8 bytes"),
    (dict(best=BEST + 4), b"after_value, best_next and delta need 8 bytes"),
    (dict(delta=DELTA + 4), b"after_value, best_next and delta need 8 bytes"),
]


@pytest.mark.parametrize("kw, message", PUSH_ERRORS, ids=[f"{list(k)[0]}: {m.decode()}" for k, m in PUSH_ERRORS])
def test_push_errors(lib, kw, message):
    a = dict(after=AFTER, value=VALUE, best=BEST, term=TERM, n=4, delta=DELTA)
    a.update(kw)
    assert lib.g2048_ntuple_delay_push(a["after"], a["value"], a["best"], a["term"], a["n"], _dl(), 0, a["delta"], None) == -1
    assert message in lib.g2048_last_error()


UPDATE_ERRORS = [
    (dict(net=None), b"net is NULL"), (dict(net=lambda staged=False: _net(T=9, staged=staged)), b"n_tuples=9"),
    (dict(net=lambda staged=False: _net(weights=None, staged=staged)), b"net weights is NULL"),
    (dict(n=0), b"n=0"), (dict(n=(1 << 32) - 255), b"n=4294967041"), (dict(shift=41), b"lr_shift=41"),
    (dict(mode=2), b"mode=2"), (dict(mode=0xffffffff), b"mode=4294967295"),
]


@pytest.mark.parametrize("kw, message", UPDATE_ERRORS, ids=[m.decode() for _, m in UPDATE_ERRORS])
def test_update_errors_in_all_four_updates(lib, kw, message):
    for k in range(1, 5):
        assert _all_calls(lib, _dl(), 0, **kw)[k] == -1 and message in lib.g2048_last_error()


@pytest.mark.parametrize("kw, message", [
    (dict(phases=0), b"phases=0"), (dict(phases=4), b"phases=4"), (dict(tc=None), b"tc is NULL"),
    (dict(tc=lambda: _tc(err=None)), b"tc err is NULL"), (dict(tc=lambda: _tc(mag=None)), b"tc mag is NULL"),
    (dict(tc=lambda: _tc(err=ERR + 4)), b"err and mag need 8 bytes")])
def test_tc_errors(lib, kw, message):
    for k in (3, 4):
        assert _all_calls(lib, _dl(), 0, **kw)[k] == -1 and message in lib.g2048_last_error()


def test_python_classes_refuse_bad_arguments():
    torch = pytest.importorskip("torch")
    import gym2048_amd
    from gym2048_amd import ntuple
    for name in ("NTupleDelay", "delayed_evaluate", "delayed_tdl_step", "delayed_tdl_train", "delayed_tcl_step", "delayed_tcl_train"):
        assert getattr(gym2048_amd, name) is getattr(ntuple, name)
    for kw in (dict(n=0), dict(n=1 << 32), dict(n=4, depth=0), dict(n=4, depth=9), dict(n=4, lam=1.5), dict(n=4, lam=-0.1),
               dict(n=4, lam=True), dict(n=4, lam="0.5")):
        with pytest.raises(ValueError):
            ntuple.NTupleDelay(device="cpu", **kw)
    dl = ntuple.NTupleDelay(4, depth=3, lam=0.25, device="cpu")
    assert "24 H + 1 bytes per board" in ntuple.NTupleDelay.__doc__
    assert dl.hist.shape == (3, 4, 16) and dl.len.shape == (4,) and dl.acc.shape == (3, 4) and dl.acc.dtype == torch.int64
    assert dl.slot == 2 and dl.lam_q16 == 16384
    assert dl.hist.numel() + dl.len.numel() + 8 * dl.acc.numel() == 4 * (24 * 3 + 1)
    good = dict(after=torch.zeros((4, 16), dtype=torch.uint8), after_value=torch.zeros(4, dtype=torch.int64),
                best_next=torch.zeros(4, dtype=torch.int64), terminated=torch.zeros(4, dtype=torch.uint8),
                out=torch.zeros(4, dtype=torch.int64))
    bad = dict(after=[torch.zeros((4, 4, 4), dtype=torch.uint8), torch.zeros((4, 16), dtype=torch.int8), torch.zeros((5, 16), dtype=torch.uint8),
                      torch.zeros((16, 4), dtype=torch.uint8).t(), torch.zeros((4, 16), dtype=torch.uint8, device="meta")],
               after_value=[torch.zeros(4, dtype=torch.int32), torch.zeros(3, dtype=torch.int64), None],
               best_next=[torch.zeros(4, dtype=torch.float64), torch.zeros((4, 1), dtype=torch.int64)],
               terminated=[torch.zeros(4, dtype=torch.int64), torch.zeros(5, dtype=torch.bool)],
               out=[torch.zeros(4, dtype=torch.int32), torch.zeros(8, dtype=torch.int64)[::2], torch.zeros(4, dtype=torch.int64, device="meta")])
    for name, values in bad.items():
        for v in values:
            with pytest.raises(ValueError, match=name):
                dl.push(**{**good, name: v})
    assert dl.slot == 2                                                  # a refused push does not advance the slot
    # state_dict: a full copy, refused when it is of another shape
    st = dl.state_dict()
    assert set(st) == {"depth", "lam_q16", "slot", "hist", "len", "acc"} and st["acc"].data_ptr() != dl.acc.data_ptr()
    for key, value in (("depth", 4), ("lam_q16", 1), ("slot", 3), ("slot", -1), ("acc", torch.zeros((3, 4), dtype=torch.int32)),
                       ("acc", torch.zeros((4, 3), dtype=torch.int64)), ("hist", torch.zeros((3, 4, 4, 4), dtype=torch.uint8)),
                       ("len", torch.zeros(4, dtype=torch.bool))):
        with pytest.raises(ValueError):
            dl.load_state_dict({**st, key: value})
    st["acc"] += 5
    st["slot"] = 1
    dl.load_state_dict(st)
    assert dl.slot == 1 and (dl.acc == 5).all()
    dl.len += 3
    dl.reset()
    assert (dl.len == 0).all() and (dl.acc == 5).all() and dl.slot == 1
    # the network's methods
    net, other = ntuple.NTupleNet(TUPLES_17x4, device="cpu"), ntuple.NTupleNet(TUPLES_17x4, device="cpu")
    w = net.weights.clone()
    tc, foreign = ntuple.NTupleTC(net), ntuple.NTupleTC(other)
    trace = ntuple.NTupleTrace(4, depth=3, device="cpu")
    meta = ntuple.NTupleDelay(4, depth=3, device="meta")
    for call in (lambda: net.delay_update(trace, 3), lambda: net.delay_update(None, 3), lambda: net.delay_update(meta, 3),
                 lambda: net.delay_update(dl, 41), lambda: net.delay_update(dl, -1), lambda: net.delay_update(dl, 3, flush=2),
                 lambda: net.delay_update(dl, 3, flush=-1), lambda: net.delay_update(dl, 3, flush="yes"),
                 lambda: net.tc_delay_update(trace, 3, tc), lambda: net.tc_delay_update(dl, 3, foreign),
                 lambda: net.tc_delay_update(dl, 3, None), lambda: net.tc_delay_update(dl, 3, tc, phases=0),
                 lambda: net.tc_delay_update(dl, 3, tc, phases=4), lambda: net.tc_delay_update(dl, 3, tc, flush=2),
                 lambda: net.tc_delay_update(meta, 3, tc), lambda: net.tc_delay_update(dl, 41, tc)):
        with pytest.raises(ValueError):
            call()
    assert torch.equal(net.weights, w) and (tc.err == 0).all() and (tc.mag == 0).all()

    # the trainers refuse a delay of another n or device, and a trace in its place, before they touch the engine
    class Engine:
        n_envs, device = 5, torch.device("cpu")

        def __getattr__(self, name):
            raise AssertionError(f"the engine was used: {name}")

    for d in (dl, trace, None, ntuple.NTupleDelay(5, device="meta")):
        for call in (lambda: ntuple.delayed_tdl_train(Engine(), net, d, 1, 3), lambda: ntuple.delayed_tcl_train(Engine(), net, tc, d, 1, 3),
                     lambda: ntuple.delayed_tdl_step(Engine(), net, d, 3), lambda: ntuple.delayed_tcl_step(Engine(), net, tc, d, 3),
                     lambda: ntuple.delayed_evaluate(Engine(), net, d, None)):
            with pytest.raises(ValueError, match="delay must be an NTupleDelay of 5 boards"):
                call()
