"""GPU: the n-tuple trace kernels (g2048_ntuple_trace_push, g2048_ntuple_trace_update, g2048_ntuple_tc_trace_update) and
the TD(lambda) / TC(lambda) trainers built on them.  Small batches equal the pure-Python reference
tests/ntuple_trace_ref.py bit for bit; large ones equal a composition of the one-step kernels (net.update / net.tc_update per
slot with d_k formed by torch integer ops), which works because phase W never changes what it reads.  Every test shows from
the reference or from its input (never from the code under test) that it reaches the edge it names.

Figures measured on the MI355X: profiles/r14_ntuple_trace_probe.txt."""
import ctypes as C

import numpy as np
import pytest

import ntuple_ref as ref
import ntuple_tc_ref as tcref
import ntuple_trace_ref as tref
from analysis_helpers import SEARCH_MAX_LANES, g, random_boards  # noqa: F401 (g: fixture)
from ntuple_helpers import TUPLES_8x4, TUPLES_17x4, random_net
from ntuple_tc_helpers import assert_tables_equal, preload
from ntuple_trace_helpers import push_inputs, trace_deltas

pytestmark = pytest.mark.gpu


def dev(torch, a):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda:0")


def device_state(g, torch, rnet, rtc=None):
    """(NTupleNet, NTupleTC or None) on the GPU with the shape and tables of a reference network and its accumulators."""
    net = g.NTupleNet(rnet.tuples, frac_bits=rnet.frac_bits, device="cuda:0")
    if not isinstance(rnet.weights, tcref.Sparse):
        net.weights.copy_(torch.as_tensor(rnet.weights.astype(np.int32)))
    if rtc is None:
        return net, None
    tc = g.NTupleTC(net)
    tc.err.copy_(torch.as_tensor(rtc.err))
    tc.mag.copy_(torch.as_tensor(rtc.mag_i64()))
    return net, tc


def tables(net, tc):
    return net.weights.cpu().numpy().astype(np.int64), tc.err.cpu().numpy(), tc.mag.cpu().numpy()


def pushed(g, torch, n, H, lam_q16, seed, pushes=12, trace=None, upto=None):
    """(device trace, reference trace) after ``pushes`` synthetic pushes, compared push by push: delta against the torch
    expression of td_evaluate and against the reference, len against the reference."""
    tr, rtr = g.NTupleTrace(n, depth=H, lam=lam_q16 / 65536), tref.Trace(n, H, lam_q16)
    assert tr.lam_q16 == lam_q16 and tr.slot == H - 1 and not tr.len.any()
    out = torch.empty(n, dtype=torch.int64, device="cuda")
    for after, av, bn, term in push_inputs(n, pushes, seed)[:upto]:
        d_av, d_bn, d_term = dev(torch, av), dev(torch, bn), dev(torch, term)
        assert tr.push(dev(torch, after), d_av, d_bn, d_term, out) is out
        want = d_bn.clone()
        want.masked_fill_(d_term.bool(), 0)
        want.sub_(d_av)
        assert torch.equal(out, want)
        assert np.array_equal(out.cpu().numpy(), tref.push(rtr, after, av, bn, term, trace))
        assert tr.slot == rtr.slot and np.array_equal(tr.len.cpu().numpy(), rtr.len)
    assert np.array_equal(tr.hist.cpu().numpy(), rtr.hist)
    return tr, rtr


@pytest.mark.parametrize("lam", [0, 32768, 65536])
@pytest.mark.parametrize("H", [1, 2, 8])
@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_small_batches_equal_the_reference(g, torch_cuda, n, H, lam):
    """Twelve pushes with synthetic termination masks -- the ring wraps, fills and clears -- then the three updates."""
    torch = torch_cuda
    ptrace = {}
    tr, rtr = pushed(g, torch, n, H, lam, 100 + n + H, trace=ptrace)
    assert ptrace["pushes"] == 12 and ptrace["wrap"] >= 1
    if n >= 63:
        assert ptrace["term"] > n and ptrace["ended"] > n and (H > 4 or ptrace["saturate"] > 0) and len(set(rtr.len.tolist())) > (1 if H == 1 else 2)
    deltas = trace_deltas(n, 7)
    rnet = random_net(TUPLES_17x4, 8, lo=-(1 << 30), hi=1 << 30)
    rtc = preload(rnet, 9, rtr.hist[rtr.slot, :8])
    d = dev(torch, deltas)
    # TD
    net, _ = device_state(g, torch, rnet)
    want, trace = rnet.copy(), {}
    tref.trace_update(want, rtr, deltas, 0, trace)
    net.trace_update(tr, d, 0)
    assert_tables_equal((net.weights.cpu().numpy().astype(np.int64),), (want.weights,))
    if n >= 63:
        assert trace["items"] > 0 and trace["sat"] > 0 and trace["zero"] > 0 and trace["clamp_d"] > 0
        assert H == 1 or (trace["short"] > 0 and (trace["items"] > n - trace["zero"]) == (lam > 0))
    # TC, both phases in one call and one phase per call
    for phases in ((3,), (1, 2)):
        net, tc = device_state(g, torch, rnet, rtc)
        want, want_tc = rnet.copy(), rtc.copy()
        tref.tc_trace_update(want, want_tc, rtr, deltas, 2, 3)
        for p in phases:
            net.tc_trace_update(tr, d, 2, tc, p)
        assert_tables_equal(tables(net, tc), (want.weights, want_tc.err, want_tc.mag_i64()))


@pytest.mark.parametrize("T", range(1, 9))
def test_every_tuple_count(g, torch_cuda, T):
    torch = torch_cuda
    n, H, lam = 65, 4, 49152
    tr, rtr = pushed(g, torch, n, H, lam, 200 + T, pushes=7)
    deltas = trace_deltas(n, 11)
    rnet = random_net(TUPLES_8x4[:T], 12, lo=-(1 << 20), hi=1 << 20)
    rtc = preload(rnet, 13)
    net, tc = device_state(g, torch, rnet, rtc)
    want = rnet.copy()
    tref.trace_update(want, rtr, deltas, 3)
    net.trace_update(tr, dev(torch, deltas), 3)
    assert_tables_equal((net.weights.cpu().numpy().astype(np.int64),), (want.weights,))
    net, tc = device_state(g, torch, rnet, rtc)
    want, want_tc = rnet.copy(), rtc.copy()
    tref.tc_trace_update(want, want_tc, rtr, deltas, 3, 3)
    net.tc_trace_update(tr, dev(torch, deltas), 3, tc)
    assert_tables_equal(tables(net, tc), (want.weights, want_tc.err, want_tc.mag_i64()))


def test_six_cell_tuple_td(g, torch_cuda):
    """T = 1, L = 6: 2^24 entries (64 MiB of weights, on the GPU only; the reference keeps the entries it wrote).  TD only:
    TC accumulators for 6-tuples are 1 GiB per table."""
    torch = torch_cuda
    tuples = ((0, 1, 2, 4, 5, 6),)
    n, H, lam = 65, 4, 32768
    tr, rtr = pushed(g, torch, n, H, lam, 301, pushes=6)
    rnet, _ = tcref.sparse_net(tuples)
    deltas = trace_deltas(n, 14)
    trace = {}
    tref.trace_update(rnet, rtr, deltas, 1, trace)
    assert trace["items"] > n and max(i for _, i in rnet.weights) >= 1 << 20
    net, _ = device_state(g, torch, rnet)
    net.trace_update(tr, dev(torch, deltas), 1)
    keys = sorted(rnet.weights)
    idx = torch.as_tensor([i for _, i in keys], device="cuda")
    vals = np.array([rnet.weights[k] for k in keys], np.int64)
    assert np.array_equal(net.weights[0, idx].cpu().numpy().astype(np.int64), vals)
    assert int(torch.count_nonzero(net.weights)) == int(np.count_nonzero(vals))          # nothing else was written


# ------------------------------------------------------------------------------------------- the composition oracle
def d_k_torch(torch, tr, delta, k):
    """d_k of every board by torch integer ops, zero where k >= L."""
    d = delta.clamp(-(1 << 40), 1 << 40)
    dk = torch.div(d * tref.decay(tr.lam_q16, k), 65536, rounding_mode="floor")          # |d * p_k| <= 2^56
    L = (tr.len & 0x7f).clamp(max=tr.depth)
    return torch.where(L > k, dk, torch.zeros_like(dk)).contiguous()


def composed(g, torch, tr, delta, lr_shift, tuples, boards_of=None):
    """(TD weights, TC weights, err, mag) by the one-step kernels: per k, net.update / tc_update(phases=1) / tc_update(
    phases=2) on the slot k pushes back with d_k."""
    H = tr.depth
    slot_boards = boards_of or (lambda k: tr.hist[(tr.slot - k) % H])
    td, tcn = g.NTupleNet(tuples), g.NTupleNet(tuples)
    tc = g.NTupleTC(tcn)
    dks = [d_k_torch(torch, tr, delta, k) for k in range(H)]
    for k in range(H):
        td.update(slot_boards(k), dks[k], lr_shift)
    for phase in (1, 2):
        for k in range(H):
            tcn.tc_update(slot_boards(k), dks[k], lr_shift, tc, phase)
    return td.weights, tcn.weights, tc.err, tc.mag


def traced(g, torch, tr, delta, lr_shift, tuples):
    td, tcn = g.NTupleNet(tuples), g.NTupleNet(tuples)
    tc = g.NTupleTC(tcn)
    td.trace_update(tr, delta, lr_shift)
    tcn.tc_trace_update(tr, delta, lr_shift, tc, 1)
    tcn.tc_trace_update(tr, delta, lr_shift, tc, 2)
    return td.weights, tcn.weights, tc.err, tc.mag


def test_composition_small_against_reference_too(g, torch_cuda):
    """The oracle itself, where the reference can check it: n = 257, H = 8."""
    torch = torch_cuda
    n, H, lam = 257, 8, 49152
    tr, rtr = pushed(g, torch, n, H, lam, 401)
    deltas = trace_deltas(n, 15)
    got = traced(g, torch, tr, dev(torch, deltas), 2, TUPLES_17x4)
    want = composed(g, torch, tr, dev(torch, deltas), 2, TUPLES_17x4)
    rnet = ref.Net(TUPLES_17x4, 10)
    tref.trace_update(rnet, rtr, deltas, 2)
    assert np.array_equal(want[0].cpu().numpy(), rnet.weights)
    for name, a, b in zip(("td weights", "tc weights", "err", "mag"), got, want):
        assert torch.equal(a, b), name


def test_composition_past_the_grid_cap(g, torch_cuda):
    """n = 2^21 + 3, H = 8: 2^24 + 24 items, more than one grid covers.  The items past the cap are k = 7 of the last 24
    boards; they have a full history and a d_7 whose step is not 0."""
    torch = torch_cuda
    n, H, lam, lr_shift = (1 << 21) + 3, 8, 49152, 4
    assert H * n > SEARCH_MAX_LANES and H * n - SEARCH_MAX_LANES == 24 and 7 * n + (n - 24) == SEARCH_MAX_LANES
    gen = torch.Generator(device="cuda").manual_seed(5)
    tr = g.NTupleTrace(n, depth=H, lam=lam / 65536)
    tr.hist.copy_(torch.randint(0, 16, (H, n, 16), generator=gen, device="cuda", dtype=torch.uint8))
    tr.len.copy_(torch.randint(0, 256, (n,), generator=gen, device="cuda", dtype=torch.uint8))     # every byte, garbage included
    tr.len[-24:] = 8
    tr.slot = 5
    delta = torch.randint(-(1 << 30), 1 << 30, (n,), generator=gen, device="cuda", dtype=torch.int64)
    delta[torch.rand(n, generator=gen, device="cuda") < 0.875] = 0
    tail = torch.arange(1, 25, device="cuda", dtype=torch.int64) << 24
    delta[-24:] = torch.where(torch.arange(24, device="cuda") % 2 == 0, tail, -tail)
    for d in delta[-24:].tolist():
        assert ref.step_of(tref.d_k(d, lam, 7), lr_shift) != 0
    got = traced(g, torch, tr, delta, lr_shift, TUPLES_17x4)
    want = composed(g, torch, tr, delta, lr_shift, TUPLES_17x4)
    for name, a, b in zip(("td weights", "tc weights", "err", "mag"), got, want):
        assert torch.equal(a, b), name
    # without the 24 items past the cap the tables would differ: their contribution alone is not zero
    only = torch.zeros_like(delta)
    only[-24:] = delta[-24:]
    alone = g.NTupleNet(TUPLES_17x4)
    alone.update(tr.hist[(tr.slot - 7) % H], d_k_torch(torch, tr, only, 7), lr_shift)
    assert bool(alone.weights.any())


def test_history_above_4_gib(g, torch_cuda):
    """n = 2^25 + 3, H = 8, one 4-tuple: hist is 4 GiB + 384 bytes.  The last 24 boards of slot 7 lie at byte
    offsets above 2^32: a push into slot 7 and the updates that read it, with delta non-zero on the first and the last five
    boards only."""
    torch = torch_cuda
    n, H = (1 << 25) + 3, 8
    tuples = ((0, 1, 4, 5),)
    tr = g.NTupleTrace(n, depth=H, lam=1.0)
    assert tr.hist.numel() > 1 << 32 and (7 * n + n - 5) * 16 >= 1 << 32     # the last five boards of slot 7 lie above 4 GiB
    ends = np.r_[0:5, n - 5:n]
    after = torch.zeros((n, 16), dtype=torch.uint8, device="cuda")
    after[dev(torch, ends)] = dev(torch, random_boards(10, 21))
    values = torch.zeros(n, dtype=torch.int64, device="cuda")
    best = torch.zeros(n, dtype=torch.int64, device="cuda")
    best[dev(torch, ends)] = dev(torch, np.array([5, -7, 9, -11, 13, -15, 17, -19, 21, -23], np.int64) << 20)
    term = torch.zeros(n, dtype=torch.uint8, device="cuda")
    term[1], term[n - 2] = 1, 0xff
    delta = torch.empty(n, dtype=torch.int64, device="cuda")
    tr.slot = 6
    tr.push(after, values, best, term, delta)
    assert tr.slot == 7
    want = best.clone()
    want[1], want[n - 2] = 0, 0
    assert torch.equal(delta, want) and int(torch.count_nonzero(delta)) == 8
    assert torch.equal(tr.hist[7, :5], after[:5]) and torch.equal(tr.hist[7, -5:], after[-5:])
    assert not tr.hist[:7].any() and int(torch.count_nonzero(tr.hist[7])) == int(torch.count_nonzero(after))
    assert int((tr.len == 1).sum()) == n - 2 and int(tr.len[1]) == 0x81 == int(tr.len[n - 2])
    got = traced(g, torch, tr, delta, 3, tuples)
    want = composed(g, torch, tr, delta, 3, tuples, boards_of=lambda k: after if k == 0 else tr.hist[(7 - k) % H])
    for name, a, b in zip(("td weights", "tc weights", "err", "mag"), got, want):
        assert torch.equal(a, b), name
    # the ten boards against the reference: every len is 1, so the update is the one-step update of those boards
    rnet = ref.Net(tuples, 10)
    ref.update(rnet, after[dev(torch, ends)].cpu().numpy(), delta[dev(torch, ends)].cpu().numpy(), 3)
    assert (rnet.weights != 0).any() and np.array_equal(got[0].cpu().numpy(), rnet.weights)


# --------------------------------------------------------------------------------------------------- engine level
ENGINE = dict(n=257, steps=800, seed=42, lr_shift=5)


def engine(g):
    eng = g.Batched2048(ENGINE["n"], seed=ENGINE["seed"])
    eng.reset()
    return eng


@pytest.fixture(scope="module")
def td0(g, torch_cuda):
    """The TD(0) run, once: (weights, max |delta| over the run, episodes finished) by td_step with the buffers of train."""
    from gym2048_amd.ntuple import td_step, td_work
    torch = torch_cuda
    net, eng = g.NTupleNet("17x4"), engine(g)
    try:
        work, worst = td_work(eng), torch.zeros((), dtype=torch.int64, device="cuda")
        for _ in range(ENGINE["steps"]):
            td_step(eng, net, ENGINE["lr_shift"], work)
            worst = torch.maximum(worst, work.delta.abs().max())
        torch.cuda.synchronize()
        return net.weights.clone(), int(worst), eng.episode_stats()["episodes"]
    finally:
        eng.close()


@pytest.fixture(scope="module")
def tc0(g, torch_cuda):
    net, eng = g.NTupleNet("17x4"), engine(g)
    tc = g.NTupleTC(net)
    try:
        g.tc_train(eng, net, tc, ENGINE["steps"], ENGINE["lr_shift"])
        torch_cuda.cuda.synchronize()
        return net.weights.clone(), tc.err.clone(), tc.mag.clone(), eng.episode_stats()["episodes"]
    finally:
        eng.close()


def test_td0_fixture_is_train_and_long_enough(g, torch_cuda, td0):
    weights, worst, episodes = td0
    assert episodes >= -(-ENGINE["n"] // 4), f"only {episodes} games finished in {ENGINE['steps']} steps: raise the step count"
    assert 0 < worst <= 1 << 40, worst
    net, eng = g.NTupleNet("17x4"), engine(g)
    try:
        g.train(eng, net, ENGINE["steps"], ENGINE["lr_shift"])
        torch_cuda.cuda.synchronize()
        assert torch_cuda.equal(net.weights, weights) and bool(weights.any())
    finally:
        eng.close()


@pytest.mark.parametrize("H, lam", [(1, 0.5), (4, 0.0)])
def test_tdl_train_with_h_1_or_lam_0_is_train(g, torch_cuda, td0, H, lam):
    weights, worst, episodes = td0
    assert worst <= 1 << 40 and episodes >= -(-ENGINE["n"] // 4)            # the equality needs |delta| <= 2^40 throughout
    net, eng = g.NTupleNet("17x4"), engine(g)
    try:
        trace = g.NTupleTrace(ENGINE["n"], depth=H, lam=lam)
        assert g.tdl_train(eng, net, trace, ENGINE["steps"], ENGINE["lr_shift"]) is net
        torch_cuda.cuda.synchronize()
        assert torch_cuda.equal(net.weights, weights)
        assert eng.episode_stats()["episodes"] == episodes
    finally:
        eng.close()


@pytest.mark.parametrize("H, lam", [(1, 0.5), (4, 0.0)])
def test_tcl_train_with_h_1_or_lam_0_is_tc_train(g, torch_cuda, tc0, H, lam):
    weights, err, mag, episodes = tc0
    assert episodes >= -(-ENGINE["n"] // 4), f"only {episodes} games finished in {ENGINE['steps']} steps: raise the step count"
    net, eng = g.NTupleNet("17x4"), engine(g)
    tc = g.NTupleTC(net)
    try:
        trace = g.NTupleTrace(ENGINE["n"], depth=H, lam=lam)
        assert g.tcl_train(eng, net, tc, trace, ENGINE["steps"], ENGINE["lr_shift"]) is net
        torch_cuda.cuda.synchronize()
        assert torch_cuda.equal(net.weights, weights) and torch_cuda.equal(tc.err, err) and torch_cuda.equal(tc.mag, mag)
        assert bool(err.any()) and eng.episode_stats()["episodes"] == episodes
    finally:
        eng.close()


def test_tdl_train_equals_the_reference_replaying_the_run(g, torch_cuda):
    """H = 4, lambda = 0.5: the afterstates, values and flags of every step are recorded from the GPU run; the reference
    pushes and updates them on the CPU (ntuple_trace_ref.trace_update_np, pinned to the scalar reference on the CPU)."""
    from gym2048_amd.ntuple import td_work, tdl_step
    torch = torch_cuda
    H, lam = 4, 32768
    net, eng = g.NTupleNet("17x4"), engine(g)
    try:
        trace, work, steps = g.NTupleTrace(ENGINE["n"], depth=H, lam=0.5), td_work(eng), []
        trace.reset()
        for _ in range(ENGINE["steps"]):
            tdl_step(eng, net, trace, ENGINE["lr_shift"], work)
            steps.append([t.cpu().numpy() for t in (work.before.after, work.before.after_value, work.after.best, eng.terminated,
                                                     work.delta)])
        episodes = eng.episode_stats()["episodes"]
        got, got_len, got_hist, got_slot = net.weights.cpu().numpy().astype(np.int64), trace.len.cpu().numpy(), trace.hist.cpu().numpy(), trace.slot
    finally:
        eng.close()
    assert episodes >= -(-ENGINE["n"] // 4), f"only {episodes} games finished in {ENGINE['steps']} steps: raise the step count"
    rnet, rtr, ptrace = ref.Net(TUPLES_17x4, 10), tref.Trace(ENGINE["n"], H, lam), {}
    for after, av, bn, term, delta in steps:
        assert np.array_equal(tref.push(rtr, after, av, bn, term, ptrace), delta)
        tref.trace_update_np(rnet, rtr, delta, ENGINE["lr_shift"])
    assert ptrace["term"] == episodes and ptrace["ended"] == ptrace["term"] - int((rtr.len & 0x80 != 0).sum()) and ptrace["saturate"] > 0
    assert got_slot == rtr.slot and np.array_equal(got_len, rtr.len) and np.array_equal(got_hist, rtr.hist)
    assert_tables_equal((got,), (rnet.weights,))


SHARDS = dict(steps=300, cut=100, H=4, lam=0.5)


def test_two_shards_with_their_own_traces_equal_the_unsharded_run(g, torch_cuda):
    """The shard protocol: evaluate (and push) everywhere, then update everywhere; for TC, W everywhere, then A everywhere."""
    from gym2048_amd.ntuple import td_work, tdl_evaluate
    torch = torch_cuda
    n, cut, H, lam, shift = ENGINE["n"], SHARDS["cut"], SHARDS["H"], SHARDS["lam"], ENGINE["lr_shift"]
    whole, eng = g.NTupleNet("17x4"), engine(g)
    whole_tc_net = g.NTupleNet("17x4")
    whole_tc = g.NTupleTC(whole_tc_net)
    try:
        g.tdl_train(eng, whole, g.NTupleTrace(n, depth=H, lam=lam), SHARDS["steps"], shift)
        boards = eng.get_boards()
    finally:
        eng.close()
    eng = engine(g)
    try:
        g.tcl_train(eng, whole_tc_net, whole_tc, g.NTupleTrace(n, depth=H, lam=lam), SHARDS["steps"], shift)
    finally:
        eng.close()
    assert bool(whole.weights.any()) and bool(whole_tc.err.any())
    for tc_form in (False, True):
        net = g.NTupleNet("17x4")
        tc = g.NTupleTC(net) if tc_form else None
        a, b = g.Batched2048(cut, seed=ENGINE["seed"]), g.Batched2048(n - cut, seed=ENGINE["seed"], board_offset=cut)
        try:
            shards = [(e, g.NTupleTrace(e.n_envs, depth=H, lam=lam), td_work(e)) for e in (a, b)]
            for e in (a, b):
                e.reset()
            for _ in range(SHARDS["steps"]):
                for e, tr, w in shards:
                    tdl_evaluate(e, net, tr, w)
                if tc_form:
                    for phase in (1, 2):
                        for e, tr, w in shards:
                            net.tc_trace_update(tr, w.delta, shift, tc, phase)
                else:
                    for e, tr, w in shards:
                        net.trace_update(tr, w.delta, shift)
            torch.cuda.synchronize()
            if tc_form:
                assert torch.equal(net.weights, whole_tc_net.weights) and torch.equal(tc.err, whole_tc.err) and torch.equal(tc.mag, whole_tc.mag)
            else:
                assert torch.equal(net.weights, whole.weights)
                assert np.array_equal(np.concatenate([a.get_boards(), b.get_boards()]), boards)
        finally:
            a.close()
            b.close()


# ---------------------------------------------------------------------------------------------------- the Python layer
def test_state_dict_round_trip_and_reset(g, torch_cuda):
    torch = torch_cuda
    tr, _ = pushed(g, torch, 50, 4, 32768, 501, upto=6)
    assert tr.hist.dtype == tr.len.dtype == torch.uint8 and tuple(tr.hist.shape) == (4, 50, 16) and tuple(tr.len.shape) == (50,)
    state = tr.state_dict()
    assert set(state) == {"depth", "lam_q16", "slot", "hist", "len"} and state["slot"] == tr.slot == 5 % 4
    assert state["hist"].data_ptr() != tr.hist.data_ptr() and bool(state["len"].any())
    other = g.NTupleTrace(50, depth=4, lam=0.5)
    ptrs = other.hist.data_ptr(), other.len.data_ptr()
    other.load_state_dict({k: v.cpu() if isinstance(v, torch.Tensor) else v for k, v in state.items()})
    assert other.slot == tr.slot and torch.equal(other.hist, tr.hist) and torch.equal(other.len, tr.len)
    assert ptrs == (other.hist.data_ptr(), other.len.data_ptr())
    tr.reset()
    assert not tr.len.any() and tr.slot == state["slot"] and bool(other.len.any())       # the snapshot is a copy
    for bad, match in ((dict(state, depth=2), "another depth or lam"), (dict(state, lam_q16=1), "another depth or lam"),
                       (dict(state, hist=state["hist"][:, :10]), "hist must be uint8"), (dict(state, len=state["len"].to(torch.int32)), "len must be uint8"),
                       (dict(state, slot=4), "slot")):
        with pytest.raises(ValueError, match=match):
            other.load_state_dict(bad)
    assert g.NTupleTrace(3, lam=1).lam_q16 == 65536 and g.NTupleTrace(3, lam=0).lam_q16 == 0 and g.NTupleTrace(3).depth == 4
    assert g.NTupleTrace(3, lam=0.3).lam_q16 == round(0.3 * 65536)


def test_bad_arguments_are_refused_and_touch_nothing(g, torch_cuda):
    torch = torch_cuda
    from gym2048_amd import _lib
    lib = _lib.load()
    n = 16
    rnet = random_net(TUPLES_17x4, 121, lo=-1000, hi=1000)
    net, tc = device_state(g, torch, rnet, preload(rnet, 122))
    tr, _ = pushed(g, torch, n, 4, 32768, 601, upto=5)
    before = tables(net, tc), tr.hist.clone(), tr.len.clone(), tr.slot
    delta = torch.full((n + 1,), 1 << 20, dtype=torch.int64, device="cuda")
    d64 = delta[:n].contiguous()
    after = dev(torch, random_boards(n, 123))
    term = torch.zeros(n, dtype=torch.uint8, device="cuda")
    out = torch.zeros(n, dtype=torch.int64, device="cuda")
    other_net = g.NTupleNet("17x4")
    elsewhere = g.NTupleTrace(n)
    elsewhere.device = torch.device("cuda:1")           # a trace that says it lives on another device
    for call, match in (
            (lambda: net.trace_update(tr, d64.to(torch.int32), 3), "delta"),
            (lambda: net.trace_update(tr, delta, 3), "delta"),
            (lambda: net.trace_update(tr, d64.cpu(), 3), "delta"),
            (lambda: net.trace_update(tr, d64, 41), "lr_shift"),
            (lambda: net.trace_update(None, d64, 3), "trace must be"),
            (lambda: net.trace_update(elsewhere, d64, 3), "weights are on"),
            (lambda: net.tc_trace_update(elsewhere, d64, 3, tc), "weights are on"),
            (lambda: net.tc_trace_update(tr, delta, 3, tc), "delta"),
            (lambda: net.tc_trace_update(tr, d64, -1, tc), "lr_shift"),
            (lambda: net.tc_trace_update(tr, d64, 3, tc, 0), "phases"),
            (lambda: net.tc_trace_update(tr, d64, 3, tc, 4), "phases"),
            (lambda: net.tc_trace_update(tr, d64, 3, None), "tc must be"),
            (lambda: net.tc_trace_update(tr, d64, 3, g.NTupleTC(other_net)), "tc must be"),
            (lambda: tr.push(after[:, :15], d64, d64, term, out), "after must be"),
            (lambda: tr.push(after, d64.to(torch.int32), d64, term, out), "after_value must be"),
            (lambda: tr.push(after, d64, delta, term, out), "best_next must be"),
            (lambda: tr.push(after, d64, d64, term.to(torch.int64), out), "terminated must be"),
            (lambda: tr.push(after, d64, d64, term, out.cpu()), "out must be"),
            (lambda: g.NTupleTrace(0), "n"), (lambda: g.NTupleTrace(4, depth=0), "depth"), (lambda: g.NTupleTrace(4, depth=9), "depth"),
            (lambda: g.NTupleTrace(4, lam=1.5), "lam"), (lambda: g.NTupleTrace(4, lam=-0.1), "lam"), (lambda: g.NTupleTrace(4, lam="x"), "lam")):
        with pytest.raises(ValueError, match=match):
            call()
    # the library refuses what gets past Python: a slot out of range
    assert lib.g2048_ntuple_trace_update(n, d64.data_ptr(), 3, C.byref(net._c), C.byref(tr._c), 4, None) == -1
    assert b"slot=4" in lib.g2048_last_error()
    torch.cuda.synchronize()
    assert_tables_equal(tables(net, tc), before[0])
    assert torch.equal(tr.hist, before[1]) and torch.equal(tr.len, before[2]) and tr.slot == before[3] and not out.any()
    assert lib.g2048_abi_version() == _lib.ABI_VERSION == 16
