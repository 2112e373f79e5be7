"""GPU: mixed-length n-tuple networks (G2048_NTUPLE_END, the NtupleMixedShape kernels) -- values,
evaluate, search, the TD(0), TC and trace updates, stages, promote and the trainers equal the reference
tests/ntuple_mixed_ref.py (the pure-Python references on a padded array) bit for bit and as whole arrays; an equal cut equals
the uniform network on the same arrays; and the real-size preset "4x6+4x4" splits into its uniform 4x6 and 4x4 halves.
Weights are full-range random int32 over the whole compact array, so a look-up one element off, or in a neighbour's table,
reads another number.  Every test shows from the reference's look-up trace or from its input (never from the code under
test) that it reaches the edge it names.  The reference is the cost: at most 67 boards at depth <= 1 (the 64 of
tests/test_gpu_ntuple_shapes.py and three edge boards), 12 at depth 2, each result computed once for the module and shared
with tests/test_ntuple_mixed_host.py.

Timings, and what was and was not measured: profiles/r18_ntuple_mixed_probe.txt."""
import numpy as np
import pytest

import ntuple_mixed_ref as mref
import ntuple_ref as ref
import ntuple_staged_ref as sref
import ntuple_trace_ref as tref
from analysis_helpers import g  # noqa: F401 (fixture)
from ntuple_helpers import TUPLES_4x6, assert_eval_equal
from ntuple_mixed_helpers import THR_3, boards_67, cached, deep, near_full_12, net_of, pushed_trace, random_tc, shallow, staged_boards, want_tables
from ntuple_search_helpers import assert_search_equal
from ntuple_tc_helpers import assert_tables_equal, edge_deltas
from ntuple_trace_helpers import trace_deltas

pytestmark = pytest.mark.gpu

NAMES = sorted(mref.SHAPES)
EDGE_STEPS = (5 << 20, -7 << 20, 3 << 20)      # the deltas of the three edge boards: each takes a step


def dev(torch, a):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda:0")


def to_np(res):
    return tuple(None if t is None else t.cpu().numpy() for t in res)


def device_state(g, torch, rnet, rtc=None):
    """(NTupleNet, NTupleTC or None) on the GPU with the lists, stages, compact weights and accumulators of a reference network."""
    flat = mref.flat_of(rnet).astype(np.int32)
    staged = len(rnet.thr) > 0
    net = g.NTupleNet(rnet.tuples, frac_bits=rnet.frac_bits, stages=rnet.thr if staged else None, mixed=True)
    assert net.mixed and tuple(net.weights.shape) == ((flat.shape if staged else flat[0].shape))
    net.weights.copy_(torch.as_tensor(flat if staged else flat[0]))
    if rtc is None:
        return net, None
    tc = g.NTupleTC(net)
    err, mag = mref.tc_flat(rtc, rnet)
    tc.err.copy_(torch.as_tensor(err if staged else err[0]))
    tc.mag.copy_(torch.as_tensor(mag if staged else mag[0]))
    return net, tc


def tables(net, tc=None):
    """The device's arrays as flat int64, as ntuple_mixed_helpers.want_tables gives the reference's."""
    w = net.weights.cpu().numpy().astype(np.int64).reshape(-1)
    return (w,) if tc is None else (w, tc.err.cpu().numpy().reshape(-1), tc.mag.cpu().numpy().reshape(-1))


def engine_with(g, boards, seed):
    eng = g.Batched2048(len(boards), seed=seed)
    eng.set_boards(boards % 32)
    eng.set_scores(np.random.default_rng(seed).integers(1, 1 << 24, len(boards)).astype(np.int32))     # deficit bits populated
    return eng


# --------------------------------------------------------------------------------- 1. the four shapes against the reference
@pytest.mark.parametrize("name", NAMES)
def test_values_evaluate_search_depth_1_plain_and_engine(g, torch_cuda, name):
    torch = torch_cuda
    boards, rnet = boards_67(), net_of(name)
    assert mref.table_edges(boards, rnet) == mref.all_edges(rnet)           # the first and last entry of each table are read
    want_v, want_e, want_s = shallow(name)
    q = want_e[0]
    assert len(set(q[60].tolist())) == 1 and q[60, 0] != ref.ILLEGAL and want_e[1][60] == 0               # the tie: smallest d
    assert (q[62] != ref.ILLEGAL).sum() == 1 and (q[63] == ref.ILLEGAL).all() and len(set(want_s[0].tolist())) == 4
    net, _ = device_state(g, torch, rnet)
    d = dev(torch, boards)
    assert np.array_equal(net.values(d).cpu().numpy(), want_v), "values"
    assert_eval_equal(to_np(net.evaluate(d)), want_e, boards, "evaluate, plain")
    assert_search_equal(to_np(net.search(d, 1)), want_s, boards, "search depth 1, plain")
    eng = engine_with(g, boards, 3)
    try:
        rec = eng.records().clone()
        assert bool((rec[:, 8:] > 31).any())
        assert_eval_equal(to_np(eng.ntuple_evaluate(net)), want_e, boards, "evaluate, engine")
        assert_search_equal(to_np(eng.ntuple_search(net, 1)), want_s, boards, "search depth 1, engine")
        assert torch.equal(eng.records(), rec)                              # the engine is left untouched
    finally:
        eng.close()


@pytest.mark.parametrize("name", NAMES)
def test_search_depth_2_plain_and_engine(g, torch_cuda, name):
    torch = torch_cuda
    boards, rnet, want = near_full_12(), net_of(name), deep(name)
    assert ((boards == 0).sum(1) <= 2).all() and (want[1][-1] == ref.ILLEGAL).all() and (want[1][:-1] != ref.ILLEGAL).any(1).all()
    net, _ = device_state(g, torch, rnet)
    assert_search_equal(to_np(net.search(dev(torch, boards), 2)), want, boards, "search depth 2, plain")
    eng = engine_with(g, boards, 4)
    try:
        rec = eng.records().clone()
        assert_search_equal(to_np(eng.ntuple_search(net, 2)), want, boards, "search depth 2, engine")
        assert torch.equal(eng.records(), rec)
    finally:
        eng.close()


@pytest.mark.parametrize("name", NAMES)
def test_update_and_tc_phases(g, torch_cuda, name):
    torch = torch_cuda
    boards, rnet = boards_67(), net_of(name)
    deltas = edge_deltas(len(boards), 93)
    deltas[64:] = EDGE_STEPS
    d, dl = dev(torch, boards), dev(torch, deltas)
    want = rnet.copy()
    sref.update(want, boards, deltas, 3)
    assert (mref.flat_of(want) != mref.flat_of(rnet)).any()
    net, _ = device_state(g, torch, rnet)
    net.update(d, dl, 3)
    assert_tables_equal(tables(net), want_tables(want))
    rtc = cached(("tc", name), lambda: random_tc(rnet, 94))
    for phases in (1, 2, 3):
        wn, wt = rnet.copy(), rtc.copy()
        sref.tc_update(wn, wt, boards, deltas, 2, phases)
        net, tc = device_state(g, torch, rnet, rtc)
        net.tc_update(d, dl, 2, tc, phases)
        assert_tables_equal(tables(net, tc), want_tables(wn, wt))


@pytest.mark.parametrize("name", NAMES)
def test_trace_updates(g, torch_cuda, name):
    torch = torch_cuda
    rnet, n = net_of(name), 24
    rtr = pushed_trace(n, 3, 40000, 95)
    assert mref.table_edges(rtr.hist[rtr.slot, :3], rnet) == mref.all_edges(rnet)
    deltas = trace_deltas(n, 96)
    deltas[:3] = EDGE_STEPS
    dl = dev(torch, deltas)
    tr = g.NTupleTrace(n, depth=3, lam=40000 / 65536)
    assert tr.lam_q16 == rtr.lam
    tr.load_state_dict({"depth": 3, "lam_q16": rtr.lam, "slot": rtr.slot, "hist": rtr.hist, "len": rtr.len})
    want = rnet.copy()
    sref.trace_update(want, rtr, deltas, 3)
    assert (mref.flat_of(want) != mref.flat_of(rnet)).any()
    net, _ = device_state(g, torch, rnet)
    net.trace_update(tr, dl, 3)
    assert_tables_equal(tables(net), want_tables(want))
    rtc = cached(("tc", name), lambda: random_tc(rnet, 94))
    wn, wt = rnet.copy(), rtc.copy()
    sref.tc_trace_update(wn, wt, rtr, deltas, 2, 3)
    net, tc = device_state(g, torch, rnet, rtc)
    net.tc_trace_update(tr, dl, 2, tc)
    assert_tables_equal(tables(net, tc), want_tables(wn, wt))


# ------------------------------------------------------------------------------------------------ 2. staged, S = 3
def test_staged_values_evaluate_search_stage_and_promote(g, torch_cuda):
    torch = torch_cuda
    boards, rnet = staged_boards(), net_of("asc", THR_3)
    trace, etrace, strace = {}, {}, {}
    want_v = sref.values_batch(boards, rnet, trace)
    stages = sref.stage_batch(boards, rnet.thr)
    assert set(trace["stage"]) == {0, 1, 2} and stages[-3:].tolist() == [0, 2, 2]                         # all S stages are read
    want_e = sref.evaluate_batch(boards, rnet, etrace)
    want_s = sref.search_batch(boards, 1, rnet, strace)
    assert etrace["after_span"] > 0 and strace["leaf_other"] > 0 and strace["chance_span"] > 0             # afterstates in other stages
    deep_b = np.concatenate([boards[np.argsort((boards == 0).sum(1), kind="stable")[:6]], near_full_12()[:4]])
    dtrace = {"memo": {}}
    want_d = sref.search_batch(deep_b, 2, rnet, dtrace)
    assert dtrace["leaf_other"] > 0
    net, _ = device_state(g, torch, rnet)
    d = dev(torch, boards)
    assert np.array_equal(net.stage(d).cpu().numpy(), stages)
    assert np.array_equal(net.values(d).cpu().numpy(), want_v)
    assert_eval_equal(to_np(net.evaluate(d)), want_e, boards, "staged evaluate, plain")
    assert_search_equal(to_np(net.search(d, 1)), want_s, boards, "staged search depth 1, plain")
    assert_search_equal(to_np(net.search(dev(torch, deep_b), 2)), want_d, deep_b, "staged search depth 2, plain")
    eng = engine_with(g, boards, 5)
    try:
        rec = eng.records().clone()
        assert_eval_equal(to_np(eng.ntuple_evaluate(net)), want_e, boards, "staged evaluate, engine")
        assert_search_equal(to_np(eng.ntuple_search(net, 1)), want_s, boards, "staged search depth 1, engine")
        assert torch.equal(eng.records(), rec)
    finally:
        eng.close()
    # promote: the boards of stage 2 then read the tables of stage 1
    rtc = cached(("tc", "asc", THR_3), lambda: random_tc(rnet, 99))
    net, tc = device_state(g, torch, rnet, rtc)
    mine = boards[stages == 2]
    want_p = ref.values_batch(mine, rnet.sub(1))
    assert len(mine) > 3 and not np.array_equal(want_p, want_v[stages == 2])
    net.promote(1, 2, tc)
    assert np.array_equal(net.values(dev(torch, mine)).cpu().numpy(), want_p)
    flat, (err, mag) = mref.flat_of(rnet), mref.tc_flat(rtc, rnet)
    assert np.array_equal(net.weights.cpu().numpy(), np.stack([flat[0], flat[1], flat[1]]))
    assert np.array_equal(tc.err.cpu().numpy(), np.stack([err[0], err[1], 0 * err[2]]))
    assert np.array_equal(tc.mag.cpu().numpy(), np.stack([mag[0], mag[1], 0 * mag[2]]))
    for t in range(4):
        assert torch.equal(net.table(t, stage=2), net.table(t, stage=1)) and net.table(t, stage=0).shape == (16 ** (t + 1),)


def test_staged_updates(g, torch_cuda):
    torch = torch_cuda
    from ntuple_staged_helpers import small_boards
    from ntuple_trace_helpers import push_inputs
    boards, rnet = staged_boards(), net_of("asc", THR_3)
    deltas = edge_deltas(len(boards), 98)
    deltas[-3:] = EDGE_STEPS
    d, dl = dev(torch, boards), dev(torch, deltas)
    want, trace = rnet.copy(), {}
    sref.update(want, boards, deltas, 3, trace)
    assert set(trace["stage"]) == {0, 1, 2} and (mref.flat_of(want) != mref.flat_of(rnet)).any(1).all()   # every set is written
    net, _ = device_state(g, torch, rnet)
    net.update(d, dl, 3)
    assert_tables_equal(tables(net), want_tables(want))
    rtc = cached(("tc", "asc", THR_3), lambda: random_tc(rnet, 99))
    for phases in (1, 2, 3):
        wn, wt = rnet.copy(), rtc.copy()
        sref.tc_update(wn, wt, boards, deltas, 2, phases)
        net, tc = device_state(g, torch, rnet, rtc)
        net.tc_update(d, dl, 2, tc, phases)
        assert_tables_equal(tables(net, tc), want_tables(wn, wt))
    n = 24
    rtr = tref.Trace(n, 3, 40000)
    pool = small_boards(n * 5, 100).reshape(5, n, 16)
    for t, (_, av, best, term) in enumerate(push_inputs(n, 5, 101)):
        tref.push(rtr, pool[t], av, best, term)
    tr = g.NTupleTrace(n, depth=3, lam=40000 / 65536)
    tr.load_state_dict({"depth": 3, "lam_q16": rtr.lam, "slot": rtr.slot, "hist": rtr.hist, "len": rtr.len})
    td = trace_deltas(n, 102)
    tdl = dev(torch, td)
    wn, wt, trace = rnet.copy(), rtc.copy(), {}
    sref.tc_trace_update(wn, wt, rtr, td, 2, 3, trace)
    assert trace["hist_span"] > 0 and set(trace["stage"]) == {0, 1, 2}      # one board's slots in different stages
    net, tc = device_state(g, torch, rnet, rtc)
    net.tc_trace_update(tr, tdl, 2, tc)
    assert_tables_equal(tables(net, tc), want_tables(wn, wt))
    wn = rnet.copy()
    sref.trace_update(wn, rtr, td, 3)
    net, _ = device_state(g, torch, rnet)
    net.trace_update(tr, tdl, 3)
    assert_tables_equal(tables(net), want_tables(wn))


# ------------------------------------------------------------------------------------------------ 3. ragged n
@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_ragged_batches(g, torch_cuda, n):
    """Batches that leave a wave partly filled: the 67 boards tiled to n rows, the reference's rows tiled alike; outputs past
    row n stay as they were."""
    torch = torch_cuda
    rnet = net_of("8")
    idx = np.arange(n) % 67
    boards = boards_67()[idx]
    want_v, want_e, want_s = shallow("8")
    net, _ = device_state(g, torch, rnet)
    d = dev(torch, boards)
    out = torch.full((n + 64,), 0x5A5A, dtype=torch.int64, device="cuda")
    net.values(d, out=out[:n])
    assert np.array_equal(out[:n].cpu().numpy(), want_v[idx]) and bool((out[n:] == 0x5A5A).all())
    assert_eval_equal(to_np(net.evaluate(d)), tuple(x[idx] for x in want_e), boards, f"evaluate, n = {n}")
    assert_search_equal(to_np(net.search(d, 1)), tuple(x[idx] for x in want_s), boards, f"search, n = {n}")
    deltas = np.random.default_rng(110 + n).integers(-(1 << 30), 1 << 30, n)
    want = rnet.copy()
    sref.update(want, boards, deltas, 4)
    net.update(d, dev(torch, deltas), 4)
    assert_tables_equal(tables(net), want_tables(want))


# ------------------------------------------------------------------------------------------------ 4. the equal cut
def cut_descriptor(net):
    """Make ``net`` (a uniform 17x4 NTupleNet) the hand-made equal cut: tuple_len = 6, every list END-padded."""
    c = net._c.net if net.stages is not None else net._c
    c.tuple_len = 6
    for t in range(5):
        c.cells[t][4] = c.cells[t][5] = mref.END
    return net


@pytest.mark.parametrize("thr", [None, THR_3], ids=["unstaged", "S=3"])
def test_equal_cut_is_the_uniform_network(g, torch_cuda, thr):
    """Every tuple cut to L' = 4 below tuple_len = 6: the layout is [T][16^4], and every output and every updated array
    equals the uniform call's -- the mixed kernels against the uniform ones on the same weight tensor contents."""
    torch = torch_cuda
    n = 65
    boards = staged_boards()[np.arange(n) % 64]
    d, dl = dev(torch, boards), dev(torch, trace_deltas(n, 120))
    shape = (5, 16 ** 4) if thr is None else (3, 5, 16 ** 4)
    w = torch.as_tensor(np.random.default_rng(121).integers(-(1 << 31), 1 << 31, size=shape).astype(np.int32)).cuda()

    def pair():
        uni, cut = g.NTupleNet("17x4", stages=thr), cut_descriptor(g.NTupleNet("17x4", stages=thr))
        uni.weights.copy_(w), cut.weights.copy_(w)
        return uni, cut, g.NTupleTC(uni), g.NTupleTC(cut)

    def same(uni, cut, tcu, tcc):
        return torch.equal(uni.weights, cut.weights) and torch.equal(tcu.err, tcc.err) and torch.equal(tcu.mag, tcc.mag)

    uni, cut, tcu, tcc = pair()
    assert torch.equal(uni.values(d), cut.values(d))
    for a, b in zip(uni.evaluate(d), cut.evaluate(d)):
        assert torch.equal(a, b)
    for depth in (1, 2):
        for a, b in zip(uni.search(d[:9], depth), cut.search(d[:9], depth)):
            assert torch.equal(a, b)
    if thr is not None:
        assert torch.equal(uni.stage(d), cut.stage(d)) and len(set(uni.stage(d).cpu().tolist())) == 3
    eng = engine_with(g, boards, 6)
    try:
        for a, b in zip(eng.ntuple_evaluate(uni), eng.ntuple_evaluate(cut)):
            assert torch.equal(a, b)
        for a, b in zip(eng.ntuple_search(uni, 1), eng.ntuple_search(cut, 1)):
            assert torch.equal(a, b)
    finally:
        eng.close()
    uni.update(d, dl, 3), cut.update(d, dl, 3)
    assert same(uni, cut, tcu, tcc) and not torch.equal(uni.weights, w)
    for _ in range(2):                                           # the second call reads the accumulators of the first
        uni.tc_update(d, dl, 2, tcu), cut.tc_update(d, dl, 2, tcc)
    assert same(uni, cut, tcu, tcc) and bool(tcu.err.any())
    tr = g.NTupleTrace(n, depth=4, lam=0.5)
    out, zero = torch.empty(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")
    for p in range(5):
        tr.push(dev(torch, np.roll(boards, p, axis=0)), zero, zero, dev(torch, (np.arange(n) + p) % 5 == 0), out)
    uni.trace_update(tr, dl, 1), cut.trace_update(tr, dl, 1)
    uni.tc_trace_update(tr, dl, 1, tcu), cut.tc_trace_update(tr, dl, 1, tcc)
    assert same(uni, cut, tcu, tcc)


# ------------------------------------------------------------------------------------------------ 5. the split, at real size
def test_preset_splits_into_its_uniform_halves(g, torch_cuda):
    """ "4x6+4x4" with device-random weights against the uniform "4x6" and 4x4 networks that hold the same tables, on 4 096
    boards of a random rollout: V adds up, q adds up less the gain counted twice, and after one update and one tc_update
    with the same deltas the compact arrays are the concatenation of the two uniform networks' arrays.  No Python reference:
    the uniform kernels are the reference (tests/test_gpu_ntuple*.py pin them)."""
    torch = torch_cuda
    n, F = 4096, 10
    from gym2048_amd.ntuple import TUPLES
    small = TUPLES["4x6+4x4"][4:]
    mixed, six, four = g.NTupleNet("4x6+4x4", frac_bits=F), g.NTupleNet("4x6", frac_bits=F), g.NTupleNet(small, frac_bits=F)
    assert mixed.mixed and mixed.n_weights == 67371008 and mixed.tuples[:4] == TUPLES_4x6 and four.tuple_len == 4
    gen = torch.Generator(device="cuda").manual_seed(130)
    mixed.weights.copy_(torch.randint(-(1 << 31), 1 << 31, (mixed.n_weights,), generator=gen, device="cuda").to(torch.int32))
    cut = 4 * 16 ** 6
    six.weights.view(-1).copy_(mixed.weights[:cut]), four.weights.view(-1).copy_(mixed.weights[cut:])
    for t in range(8):
        assert torch.equal(mixed.table(t), (six.table(t) if t < 4 else four.table(t - 4)))
    eng = g.Batched2048(n, seed=131)
    try:
        eng.reset()
        for _ in range(150):
            eng.step(None)                                        # the synthetic random policy, auto-reset
        boards = torch.as_tensor(eng.get_boards().reshape(n, 16)).cuda()
    finally:
        eng.close()
    assert len(torch.unique(boards, dim=0)) > n // 8 and int(boards.max()) >= 5     # many distinct boards, tiles up to 32 and beyond
    assert torch.equal(mixed.values(boards), six.values(boards) + four.values(boards))
    zero = g.NTupleNet(((0,),), frac_bits=F)                     # all weights 0: q[d] = gain_d << F on the legal d
    qm, q6, q4, gain = (net.evaluate(boards).value for net in (mixed, six, four, zero))
    legal = gain != ref.ILLEGAL
    assert bool(legal.any(1).all()) and bool((~legal).any()) and bool((gain[legal] > 0).any())
    assert torch.equal(qm[legal], q6[legal] + q4[legal] - gain[legal]) and bool((qm[~legal] == ref.ILLEGAL).all())
    deltas = torch.randint(-(1 << 34), 1 << 34, (n,), generator=gen, device="cuda")
    deltas[::7] = 0
    before = mixed.weights.clone()
    for net in (mixed, six, four):
        net.update(boards, deltas, 4)
    assert not torch.equal(mixed.weights, before)
    assert torch.equal(mixed.weights[:cut], six.weights.view(-1)) and torch.equal(mixed.weights[cut:], four.weights.view(-1))
    tcs = [g.NTupleTC(net) for net in (mixed, six, four)]
    for _ in range(2):                                            # the second call reads the accumulators of the first
        for net, tc in zip((mixed, six, four), tcs):
            net.tc_update(boards, deltas, 3, tc)
    assert torch.equal(mixed.weights[:cut], six.weights.view(-1)) and torch.equal(mixed.weights[cut:], four.weights.view(-1))
    for name in ("err", "mag"):
        m, a, b = (getattr(tc, name) for tc in tcs)
        assert bool(m.any()) and torch.equal(m[:cut], a.view(-1)) and torch.equal(m[cut:], b.view(-1))


# ------------------------------------------------------------------------------------------------ 6. trainers
def test_trainer_steps_equal_the_reference(g, torch_cuda):
    """Three td_step and three tcl_step on a 16-board engine with staged MIX_ASC (S = 2), the reference stepped alongside;
    then one train(..., carousel=...) step twice from the same state: the same bits."""
    torch = torch_cuda
    from gym2048_amd.ntuple import tcl_step, td_step, train
    n, seed, shift, H = 16, 42, 4, 4
    thr = (sref.stage_mask(4),)
    flat = np.random.default_rng(140).integers(-(1 << 20), 1 << 20, size=(2, mref.n_weights(mref.MIX_ASC))).astype(np.int32)
    rnet, trace = mref.mixed_net(mref.MIX_ASC, thr, 10, flat), {}
    rtc, rtr = mref.tc_of(rnet), tref.Trace(n, H, 32768)
    net, tc = device_state(g, torch, rnet, rtc)
    envs = ref.make_envs(n, seed)
    eng = g.Batched2048(n, seed=seed)
    try:
        eng.reset()
        tr = g.NTupleTrace(n, depth=H, lam=0.5)
        for _ in range(3):
            td_step(eng, net, shift)
            sref.td_step(envs, rnet, shift, trace)
        for _ in range(3):
            tcl_step(eng, net, tc, tr, shift)
            sref.tcl_step(envs, rnet, rtc, rtr, shift, trace)
        torch.cuda.synchronize()
        assert len(trace["stage"]) == 2 and trace["after_span"] > 0
        assert_tables_equal(tables(net, tc), want_tables(rnet, rtc))        # weights, err and mag equal the reference's
        assert np.array_equal(eng.get_boards().reshape(-1, 16), np.array([ref.env_board(e) for e in envs], np.uint8))
        assert np.array_equal(tr.hist.cpu().numpy(), rtr.hist) and np.array_equal(tr.len.cpu().numpy(), rtr.len)
    finally:
        eng.close()

    def carousel_run():
        other, _ = device_state(g, torch, rnet)
        e = g.Batched2048(n, seed=seed)
        try:
            e.reset()
            car = g.Carousel(other, n, capacity=8, seed=7)
            train(e, other, 1, shift, carousel=car)
            torch.cuda.synchronize()
            return other.weights.clone(), e.records().clone(), car.pool.clone(), car.count.clone()
        finally:
            e.close()

    first, second = carousel_run(), carousel_run()
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    assert not torch.equal(first[0], torch.as_tensor(mref.flat_of(rnet).astype(np.int32)).cuda())
