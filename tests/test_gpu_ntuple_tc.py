"""GPU: the temporal-coherence kernels (g2048_ntuple_tc_update_plain, phases W and A) and the trainer built on them equal
the pure-Python reference tests/ntuple_tc_ref.py bit for bit on weights, err and mag.  Every test shows from the reference
(never from the code under test) that its input reaches the edge it names.

Figures measured on the MI355X: profiles/r13_ntuple_tc_probe.txt."""
import ctypes as C

import numpy as np
import pytest

import ntuple_ref as ref
import ntuple_tc_ref as tcref
from analysis_helpers import SEARCH_MAX_LANES, g, mixed_boards, random_boards, tiled  # noqa: F401 (g: fixture)
from ntuple_helpers import TUPLES_17x4, random_net
from ntuple_tc_helpers import EDGE_PAIRS, assert_tables_equal, edge_deltas, preload

pytestmark = pytest.mark.gpu


def dev(torch, a):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda:0")


def device_state(g, torch, rnet, rtc):
    """(NTupleNet, NTupleTC) on the GPU with the shape and tables of a reference network and its accumulators."""
    net = g.NTupleNet(rnet.tuples, frac_bits=rnet.frac_bits, device="cuda:0")
    net.weights.copy_(torch.as_tensor(rnet.weights.astype(np.int32)))
    tc = g.NTupleTC(net)
    tc.err.copy_(torch.as_tensor(rtc.err))
    tc.mag.copy_(torch.as_tensor(rtc.mag_i64()))
    return net, tc


def tables(net, tc):
    return net.weights.cpu().numpy().astype(np.int64), tc.err.cpu().numpy(), tc.mag.cpu().numpy()


def want_tables(rnet, rtc):
    return rnet.weights, rtc.err, rtc.mag_i64()


@pytest.mark.parametrize("phases", [3, 1, 2])
def test_edges_of_rate_and_step(g, torch_cuda, phases):
    """One batch on the 17x4 network with accumulators pre-loaded so that every edge of the definition is met."""
    torch = torch_cuda
    boards = mixed_boards(300, 61)
    rnet = random_net(TUPLES_17x4, 62, lo=-(1 << 30), hi=1 << 30)
    rtc = preload(rnet, 63, boards[:8])
    deltas = edge_deltas(len(boards), 64)
    net, tc = device_state(g, torch, rnet, rtc)
    trace = {}
    tcref.tc_update(rnet, rtc, boards, deltas, 0, phases, trace)
    assert trace["zero"] >= 30 and trace["clamp_d"] >= 4 and trace["multi"] > 100
    if phases & 1:
        assert trace["k"] > 1000 and trace["rate0"] > 100 and trace["rate1"] > 1000 and trace["clamp_m"] >= 3
        assert trace["sat"] > 0 and trace["zero_step"] > 0
    net.tc_update(dev(torch, boards), dev(torch, deltas), 0, tc, phases)
    assert_tables_equal(tables(net, tc), want_tables(rnet, rtc))


def test_wide_tables_offsets_above_2_16(g, torch_cuda):
    """T = 1, L = 6: 2^24 entries per table (268 MiB of tables, on the GPU only; the reference keeps the entries it wrote)."""
    torch = torch_cuda
    tuples = ((0, 1, 2, 4, 5, 6),)
    rnet, rtc = tcref.sparse_net(tuples)
    boards = np.concatenate([random_boards(150, 71), np.array([[15, 16, 17, 31] * 4], np.uint8)])
    hits = [h for b in boards for h in tcref.hits_of(b, rnet)]
    assert max(i for _, i in hits) == 16 ** 6 - 1 and sum(i >= 1 << 16 for _, i in hits) > len(hits) // 2
    net = g.NTupleNet(tuples, device="cuda:0")
    tc = g.NTupleTC(net)
    assert tuple(tc.err.shape) == tuple(tc.mag.shape) == (1, 16 ** 6)
    for k, (t, i) in enumerate(hits[:64]):              # a few accumulators at the edges of the rate
        e, a = EDGE_PAIRS[k % len(EDGE_PAIRS)]
        rtc.err[t, i], rtc.mag[t, i] = e, a
        tc.err[t, i], tc.mag[t, i] = e, a - (1 << 64) if a >= 1 << 63 else a
    d = dev(torch, boards)
    trace = {}
    for seed, shift in ((72, 0), (73, 3)):              # the second call learns at the rates the first one left
        deltas = edge_deltas(len(boards), seed)
        tcref.tc_update(rnet, rtc, boards, deltas, shift, 3, trace)
        net.tc_update(d, dev(torch, deltas), shift, tc, 3)
    assert trace["k"] > 0 and 0 < trace["rate1"] < 2 * len(hits) and trace["rate0"] > 0
    for name, got, want in (("weights", net.weights, rnet.weights), ("err", tc.err, rtc.err), ("mag", tc.mag, rtc.mag)):
        keys = sorted(want)
        idx = torch.as_tensor([i for _, i in keys], device="cuda")
        vals = np.array([want[k] - (1 << 64) if want[k] >= 1 << 63 else want[k] for k in keys], np.int64)   # mag: the int64 pattern
        assert np.array_equal(got[0, idx].cpu().numpy().astype(np.int64), vals), name
        assert int(torch.count_nonzero(got)) == int(np.count_nonzero(vals)), name     # nothing else was written


def test_contention_every_hit_reads_the_accumulators_of_before_the_call(g, torch_cuda):
    """4 096 copies of one board with mixed-sign deltas in one call: every lane's rate comes from the accumulators as they
    were before the call, not from what other lanes of the call have added."""
    torch = torch_cuda
    n = 4096
    board = np.array([[1, 2, 0, 0, 2, 1, 0, 0, 0, 0, 3, 0, 0, 0, 0, 3]], np.uint8)   # equal to its transpose: entries read twice
    boards = np.repeat(board, n, axis=0)
    rnet = random_net(TUPLES_17x4, 81, lo=-1000, hi=1000)
    rtc = tcref.TC(rnet)                                 # zero accumulators: rate 1.0 for every hit of the call
    hits = tcref.hits_of(board, rnet)
    assert len(set(hits)) < len(hits)
    deltas = np.random.default_rng(82).integers(-(1 << 16), 1 << 16, n)
    assert (deltas > 0).sum() > 1000 and (deltas < 0).sum() > 1000
    net, tc = device_state(g, torch, rnet, rtc)
    whole, whole_tc, trace = rnet.copy(), rtc.copy(), {}
    tcref.tc_update(whole, whole_tc, boards, deltas, 4, 3, trace)
    assert trace["rate1"] == n * len(hits)
    # the other semantics -- each board sees what the boards before it added -- gives other weights for this input
    serial, serial_tc = rnet.copy(), rtc.copy()
    for b, dl in zip(boards, deltas):
        tcref.tc_update(serial, serial_tc, b, [dl], 4, 3)
    assert (serial.weights != whole.weights).any() and (serial_tc.err == whole_tc.err).all()
    net.tc_update(dev(torch, boards), dev(torch, deltas), 4, tc, 3)
    assert_tables_equal(tables(net, tc), want_tables(whole, whole_tc))


def test_w_on_both_halves_then_a_on_both_halves_is_the_whole_call(g, torch_cuda):
    torch = torch_cuda
    half = mixed_boards(200, 91)
    boards = np.concatenate([half, half[::-1]])          # the halves reach the same entries
    cut = len(half)
    rnet = random_net(TUPLES_17x4, 92, lo=-(1 << 20), hi=1 << 20)
    rtc = preload(rnet, 93)
    deltas = np.random.default_rng(94).integers(-(1 << 30), 1 << 30, len(boards))
    whole, whole_tc = rnet.copy(), rtc.copy()
    tcref.tc_update(whole, whole_tc, boards, deltas, 5, 3)
    # phases = 3 on the halves in sequence is something else: the second half sees the first half's accumulators
    seq, seq_tc = rnet.copy(), rtc.copy()
    tcref.tc_update(seq, seq_tc, boards[:cut], deltas[:cut], 5, 3)
    tcref.tc_update(seq, seq_tc, boards[cut:], deltas[cut:], 5, 3)
    assert (seq.weights != whole.weights).any() and (seq_tc.err == whole_tc.err).all() and (seq_tc.mag == whole_tc.mag).all()
    d, dl = dev(torch, boards), dev(torch, deltas)
    parts = [(d[:cut].contiguous(), dl[:cut].contiguous()), (d[cut:].contiguous(), dl[cut:].contiguous())]
    net, tc = device_state(g, torch, rnet, rtc)
    for phase in (1, 2):
        for b, x in parts:
            net.tc_update(b, x, 5, tc, phase)
    assert_tables_equal(tables(net, tc), want_tables(whole, whole_tc))
    net, tc = device_state(g, torch, rnet, rtc)
    net.tc_update(d, dl, 5, tc)                          # phases defaults to 3
    assert_tables_equal(tables(net, tc), want_tables(whole, whole_tc))
    net, tc = device_state(g, torch, rnet, rtc)
    for b, x in parts:
        net.tc_update(b, x, 5, tc, 3)
    assert_tables_equal(tables(net, tc), want_tables(seq, seq_tc))


def test_grid_stride_passes(g, torch_cuda):
    """n lanes past the grid cap: the boards after the first pass are reached by the kernels' stride loop.  Only the last
    pass and one board of the first have a delta, so the reference stays small."""
    torch = torch_cuda
    n, m = SEARCH_MAX_LANES + 1027, 509
    assert n > SEARCH_MAX_LANES and n % m != 0
    base = mixed_boards(m, 101)
    live = np.concatenate([[5], np.arange(SEARCH_MAX_LANES, n)])
    values = np.random.default_rng(102).integers(-(1 << 24), 1 << 24, len(live))
    values[values == 0] = 1
    rnet = random_net(TUPLES_17x4, 103, lo=-(1 << 20), hi=1 << 20)
    rtc = preload(rnet, 104)
    net, tc = device_state(g, torch, rnet, rtc)
    tcref.tc_update(rnet, rtc, base[live % m], values, 2, 3)
    deltas = torch.zeros(n, dtype=torch.int64, device="cuda")
    deltas[dev(torch, live)] = dev(torch, values)
    net.tc_update(tiled(torch, base, n).contiguous(), deltas, 2, tc, 3)
    assert_tables_equal(tables(net, tc), want_tables(rnet, rtc))


TRAIN = dict(n=64, steps=40, seed=42, lr_shift=5)


@pytest.fixture(scope="module")
def trained():
    """The reference TC trainer on oracle.cpu_ref boards: (network, accumulators, boards, scores, trace), once."""
    rnet, trace = ref.Net(TUPLES_17x4, 10), {}
    rtc = tcref.TC(rnet)
    envs = ref.make_envs(TRAIN["n"], TRAIN["seed"])
    for _ in range(TRAIN["steps"]):
        tcref.tc_step(envs, rnet, rtc, TRAIN["lr_shift"], trace)
    return rnet, rtc, np.array([ref.env_board(e) for e in envs], np.uint8), np.array([e.score for e in envs]), trace


def test_tc_train_equals_the_reference_trainer(g, torch_cuda, trained):
    torch = torch_cuda
    rnet, rtc, boards, scores, trace = trained
    assert (rnet.weights != 0).any() and (rtc.err != 0).any() and trace["multi"] > 0 and 0 < trace["rate1"] and trace["rate0"] + trace["zero_step"] > 0
    assert ((rtc.mag > 0) & (np.abs(rtc.err).astype(np.uint64) < rtc.mag)).any()       # some weight has slowed down
    net = g.NTupleNet("17x4", frac_bits=10)
    tc = g.NTupleTC(net)
    eng = g.Batched2048(TRAIN["n"], seed=TRAIN["seed"])
    try:
        eng.reset()
        assert g.tc_train(eng, net, tc, TRAIN["steps"], TRAIN["lr_shift"]) is net
        torch.cuda.synchronize()
        assert_tables_equal(tables(net, tc), want_tables(rnet, rtc))
        assert np.array_equal(eng.get_boards().reshape(-1, 16), boards) and np.array_equal(eng.get_scores(), scores)
        assert eng.episode_stats()["episodes"] == trace["episodes"]
    finally:
        eng.close()


def test_two_shards_sharing_net_and_accumulators_equal_the_unsharded_run(g, torch_cuda, trained):
    """The shard protocol: evaluate everywhere, W everywhere, A everywhere."""
    from gym2048_amd.ntuple import tc_update, td_evaluate, td_work
    torch = torch_cuda
    rnet, rtc, boards, scores, _ = trained
    net = g.NTupleNet("17x4", frac_bits=10)
    tc = g.NTupleTC(net)
    cut = 24
    a, b = g.Batched2048(cut, seed=TRAIN["seed"]), g.Batched2048(TRAIN["n"] - cut, seed=TRAIN["seed"], board_offset=cut)
    try:
        works = [td_work(e) for e in (a, b)]
        for e in (a, b):
            e.reset()
        for _ in range(TRAIN["steps"]):
            for e, w in zip((a, b), works):
                td_evaluate(e, net, w)
            for phase in (1, 2):
                for w in works:
                    tc_update(net, tc, w, TRAIN["lr_shift"], phase)
        torch.cuda.synchronize()
        assert_tables_equal(tables(net, tc), want_tables(rnet, rtc))
        assert np.array_equal(np.concatenate([a.get_boards(), b.get_boards()]).reshape(-1, 16), boards)
        assert np.array_equal(np.concatenate([a.get_scores(), b.get_scores()]), scores)
    finally:
        a.close()
        b.close()


def test_state_dict_round_trip(g, torch_cuda):
    torch = torch_cuda
    net = g.NTupleNet("17x4")
    tc = g.NTupleTC(net)
    assert tc.err.dtype == tc.mag.dtype == torch.int64 and tuple(tc.err.shape) == tuple(tc.mag.shape) == (5, 16 ** 4)
    assert tc.err.device == tc.mag.device == net.weights.device and not tc.err.any() and not tc.mag.any()
    boards = dev(torch, random_boards(50, 111))
    net.tc_update(boards, dev(torch, np.arange(-25, 25) * 1000), 3, tc)
    state = tc.state_dict()
    assert set(state) == {"err", "mag"} and state["err"].data_ptr() != tc.err.data_ptr() and bool(state["mag"].any())
    other = g.NTupleTC(net)
    ptrs = other.err.data_ptr(), other.mag.data_ptr()
    other.load_state_dict({k: v.cpu() for k, v in state.items()})
    assert torch.equal(other.err, tc.err) and torch.equal(other.mag, tc.mag) and ptrs == (other.err.data_ptr(), other.mag.data_ptr())
    net.tc_update(boards, dev(torch, np.arange(-25, 25) * 7), 3, tc)     # the snapshot is a copy
    assert torch.equal(other.err, state["err"]) and not torch.equal(tc.err, state["err"])
    with pytest.raises(ValueError, match="err must be int64"):
        other.load_state_dict({"err": state["err"].to(torch.int32), "mag": state["mag"]})
    with pytest.raises(ValueError, match="mag must be int64"):
        other.load_state_dict({"err": state["err"], "mag": state["mag"][:, :16]})


def test_bad_arguments_are_refused_and_touch_nothing(g, torch_cuda):
    torch = torch_cuda
    from gym2048_amd import _lib
    lib = _lib.load()
    rnet = random_net(TUPLES_17x4, 121, lo=-1000, hi=1000)
    net, tc = device_state(g, torch, rnet, preload(rnet, 122))
    before = tables(net, tc)
    n = 16
    boards = dev(torch, random_boards(n, 123))
    delta = torch.full((n + 1,), 1 << 20, dtype=torch.int64, device="cuda")
    B, D, N, T = boards.data_ptr(), delta.data_ptr(), C.byref(net._c), C.byref(tc._c)

    def tcc(err=tc.err.data_ptr(), mag=tc.mag.data_ptr()):
        return C.byref(_lib.NTupleTCC(err, mag))

    bad_net = _lib.NTupleNetC(9, 4, 10)
    bad_net.weights = net.weights.data_ptr()
    cases = [
        (lambda: lib.g2048_ntuple_tc_update_plain(None, n, D, 3, 3, N, T, None), b"boards is NULL"),
        (lambda: lib.g2048_ntuple_tc_update_plain(B + 8, n, D, 3, 3, N, T, None), b"boards need 16 bytes"),
        (lambda: lib.g2048_ntuple_tc_update_plain(B, 0, D, 3, 3, N, T, None), b"n=0"),
        (lambda: lib.g2048_ntuple_tc_update_plain(B, 1 << 32, D, 3, 3, N, T, None), b"n=4294967296"),
        (lambda: lib.g2048_ntuple_tc_update_plain(B, n, D, 3, 3, None, T, None), b"net is NULL"),
        (lambda: lib.g2048_ntuple_tc_update_plain(B, n, D, 3, 3, C.byref(bad_net), T, None), b"n_tuples=9"),
        (lambda: lib.g2048_ntuple_tc_update_plain(B, n, None, 3, 3, N, T, None), b"delta is NULL"),
        (lambda: lib.g2048_ntuple_tc_update_plain(B, n, D + 4, 3, 3, N, T, None), b"delta needs 8 bytes"),
        (lambda: lib.g2048_ntuple_tc_update_plain(B, n, D, 41, 3, N, T, None), b"lr_shift=41"),
        (lambda: lib.g2048_ntuple_tc_update_plain(B, n, D, 3, 0, N, T, None), b"phases=0"),
        (lambda: lib.g2048_ntuple_tc_update_plain(B, n, D, 3, 4, N, T, None), b"phases=4"),
        (lambda: lib.g2048_ntuple_tc_update_plain(B, n, D, 3, 3, N, None, None), b"tc is NULL"),
        (lambda: lib.g2048_ntuple_tc_update_plain(B, n, D, 3, 3, N, tcc(err=None), None), b"tc err is NULL"),
        (lambda: lib.g2048_ntuple_tc_update_plain(B, n, D, 3, 3, N, tcc(mag=None), None), b"tc mag is NULL"),
        (lambda: lib.g2048_ntuple_tc_update_plain(B, n, D, 3, 3, N, tcc(err=tc.err.data_ptr() + 4), None), b"err and mag need 8 bytes"),
        (lambda: lib.g2048_ntuple_tc_update_plain(B, n, D, 3, 3, N, tcc(mag=tc.mag.data_ptr() + 4), None), b"err and mag need 8 bytes"),
    ]
    for call, message in cases:
        assert call() == -1 and message in lib.g2048_last_error(), message      # G2048_ERR_INVALID
    # the Python layer refuses before the library
    d64 = delta[:n].contiguous()
    other = g.NTupleNet("17x4")
    for call, match in (
            (lambda: net.tc_update(boards, d64.to(torch.int32), 3, tc), "delta"),
            (lambda: net.tc_update(boards, delta, 3, tc), "delta"),
            (lambda: net.tc_update(boards, d64.cpu(), 3, tc), "delta"),
            (lambda: net.tc_update(boards.cpu(), d64, 3, tc), "boards"),
            (lambda: net.tc_update(boards.to(torch.int32), d64, 3, tc), "boards"),
            (lambda: net.tc_update(boards[:, :15], d64, 3, tc), "boards"),
            (lambda: net.tc_update(boards, d64, 41, tc), "lr_shift"),
            (lambda: net.tc_update(boards, d64, -1, tc), "lr_shift"),
            (lambda: net.tc_update(boards, d64, 3.0, tc), "lr_shift"),
            (lambda: net.tc_update(boards, d64, 3, tc, 0), "phases"),
            (lambda: net.tc_update(boards, d64, 3, tc, 4), "phases"),
            (lambda: net.tc_update(boards, d64, 3, tc, True), "phases"),
            (lambda: net.tc_update(boards, d64, 3, None), "tc must be"),
            (lambda: net.tc_update(boards, d64, 3, g.NTupleTC(other)), "tc must be"),
            (lambda: g.NTupleTC(None), "net must be")):
        with pytest.raises(ValueError, match=match):
            call()
    torch.cuda.synchronize()
    assert_tables_equal(tables(net, tc), before)
    assert lib.g2048_abi_version() == _lib.ABI_VERSION == 16
