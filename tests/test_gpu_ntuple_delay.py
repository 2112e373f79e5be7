"""GPU: the n-tuple delay kernels (g2048_ntuple_delay_push, g2048_ntuple_delay_update, g2048_ntuple_tc_delay_update and
their staged siblings) and the delayed TD(lambda) / TC(lambda) trainers built on them.  Small batches equal the pure-Python
reference tests/ntuple_delay_ref.py bit for bit -- ring, accumulators and delta after every push, tables after every update;
large ones equal a composition of the one-step kernels with D gathered by torch integer ops.  The four consequences of
INTEGRATION.md §19 each have a test.  Every test shows from the reference or from its input (never from the code under test)
that it reaches the edge it names.

Figures measured on the MI355X: profiles/r22_ntuple_delay_probe.txt."""
import ctypes as C

import numpy as np
import pytest

import ntuple_delay_ref as dref
import ntuple_mixed_ref as mref
import ntuple_ref as ref
import ntuple_staged_ref as sref
import ntuple_tc_ref as tcref
from analysis_helpers import SEARCH_MAX_LANES, g, random_boards  # noqa: F401 (g: fixture)
from ntuple_helpers import TUPLES_8x4, TUPLES_17x4
from ntuple_mixed_helpers import THR_3, random_tc, want_tables
from ntuple_staged_helpers import small_boards
from ntuple_tc_helpers import assert_tables_equal
from ntuple_trace_helpers import push_inputs
from ntuple_update_matrix import assert_ring_equal, dev, device_state, ref_net, run_against_reference, tables

pytestmark = pytest.mark.gpu
MAXD = 1 << 40


def push_both(torch, dl, rdl, out, after, av, bn, term, where=""):
    assert dl.push(dev(torch, after), dev(torch, av), dev(torch, bn), dev(torch, term), out) is out
    want = dref.push(rdl, after, av, bn, term)
    assert np.array_equal(out.cpu().numpy(), want), f"{where}: delta"
    assert_ring_equal(dl, rdl, where)
    return want


@pytest.mark.parametrize("lam", [0, 32768, 65536])
@pytest.mark.parametrize("H", [1, 2, 8])
@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_small_batches_equal_the_reference(g, torch_cuda, n, H, lam):
    """Twelve pushes with synthetic termination masks -- the ring wraps, fills and clears; deltas up to 2^41, so both clamps
    bite."""
    applied, rdl = run_against_reference(g, torch_cuda, n, H, lam, ref_net(TUPLES_17x4, 8), 12, 100 + n + H)
    assert (applied[dref.FLUSH] == 0) == (H == 1)
    if n >= 63 and H > 1:
        assert applied[dref.FLUSH] < n * (H - 1)                                   # some boards had ended at the last push


def test_h_1_is_the_trace_update_at_h_1(g, torch_cuda):
    """Consequence 2, TD and TC, push by push on a second network with an NTupleTrace."""
    torch = torch_cuda
    n, rnet = 65, ref_net(TUPLES_17x4, 20)
    rtc = random_tc(rnet, 21)
    (a, _), (b, _) = device_state(g, torch, rnet), device_state(g, torch, rnet)
    (ta, tca), (tb, tcb) = device_state(g, torch, rnet, rtc), device_state(g, torch, rnet, rtc)
    dl, tr = g.NTupleDelay(n, depth=1, lam=0.5), g.NTupleTrace(n, depth=1, lam=0.5)
    d1, d2 = torch.empty(n, dtype=torch.int64, device="cuda"), torch.empty(n, dtype=torch.int64, device="cuda")
    for after, av, bn, term in push_inputs(n, 5, 22, span=1 << 41):
        args = [dev(torch, x) for x in (after, av, bn, term)]
        dl.push(*args, d1)
        tr.push(*args, d2)
        assert torch.equal(d1, d2) and torch.equal(dl.len, tr.len) and torch.equal(dl.hist, tr.hist) and int(d1.abs().max()) > MAXD
        a.delay_update(dl, 9)
        b.trace_update(tr, d2, 9)
        ta.tc_delay_update(dl, 9, tca)
        tb.tc_trace_update(tr, d2, 9, tcb)
        assert torch.equal(a.weights, b.weights) and torch.equal(ta.weights, tb.weights)
        assert torch.equal(tca.err, tcb.err) and torch.equal(tca.mag, tcb.mag)
    before = a.weights.clone()
    a.delay_update(dl, 9, flush=True)                                              # nothing is ever pending at H = 1
    assert torch.equal(a.weights, before) and not torch.equal(before, dev(torch, mref.flat_of(rnet).astype(np.int32)).reshape(before.shape))


def test_lambda_0_equals_the_plain_updates_after_the_flush(g, torch_cuda):
    """Consequence 3: H = 4, lambda = 0, every |delta| <= 2^40."""
    torch = torch_cuda
    n, rnet = 65, ref_net(TUPLES_17x4, 30)
    (a, _), (b, _) = device_state(g, torch, rnet), device_state(g, torch, rnet)
    dl = g.NTupleDelay(n, depth=4, lam=0.0)
    delta = torch.empty(n, dtype=torch.int64, device="cuda")
    for after, av, bn, term in push_inputs(n, 12, 31, span=1 << 39):
        dl.push(dev(torch, after), dev(torch, av), dev(torch, bn), dev(torch, term), delta)
        assert 0 < int(delta.abs().max()) <= MAXD
        a.delay_update(dl, 7)
        b.update(dev(torch, after), delta, 7)
    assert not torch.equal(a.weights, b.weights)                                   # errors are still pending ...
    a.delay_update(dl, 7, flush=True)
    assert torch.equal(a.weights, b.weights)                                       # ... and the flush applies exactly those


@pytest.mark.parametrize("T", range(1, 9))
def test_every_tuple_count(g, torch_cuda, T):
    run_against_reference(g, torch_cuda, 65, 4, 49152, ref_net(TUPLES_8x4[:T], 40 + T), 7, 200 + T)


def test_six_cell_tuple_td(g, torch_cuda):
    """T = 1, L = 6: 2^24 entries (64 MiB of weights, on the GPU only; the reference keeps the entries it wrote).  TD only:
    TC accumulators for 6-tuples are 1 GiB per table."""
    torch = torch_cuda
    tuples = ((0, 1, 2, 4, 5, 6),)
    n, H = 65, 4
    rnet, _ = tcref.sparse_net(tuples)
    net = g.NTupleNet(tuples)
    dl, rdl = g.NTupleDelay(n, depth=H, lam=0.5), dref.Delay(n, H, 32768)
    out = torch.empty(n, dtype=torch.int64, device="cuda")
    for t, (after, av, bn, term) in enumerate(push_inputs(n, 6, 301)):
        push_both(torch, dl, rdl, out, after, av, bn, term, f"push {t}")
        net.delay_update(dl, 1)
        boards, Ds = dref.due_items(rdl, dref.STEP)
        ref.update(rnet, boards, Ds, 1)
    net.delay_update(dl, 1, flush=True)
    ref.update(rnet, *dref.due_items(rdl, dref.FLUSH), 1)
    keys = sorted(rnet.weights)
    assert len(keys) > n and max(i for _, i in keys) >= 1 << 20
    idx = torch.as_tensor([i for _, i in keys], device="cuda")
    vals = np.array([rnet.weights[k] for k in keys], np.int64)
    assert np.array_equal(net.weights[0, idx].cpu().numpy().astype(np.int64), vals)
    assert int(torch.count_nonzero(net.weights)) == int(np.count_nonzero(vals))    # nothing else was written


def test_staged_network_whose_pushes_cross_a_stage_boundary(g, torch_cuda):
    n, H, pushes = 67, 4, 7
    boards = small_boards(n * pushes, 50).reshape(pushes, n, 16)
    rnet = ref_net(TUPLES_8x4[:3], 51, THR_3)
    stages = np.array([sref.stage_batch(b, THR_3) for b in boards])                # [pushes, n]
    assert set(stages.reshape(-1).tolist()) == {0, 1, 2}
    assert ((stages[-H:] != stages[-1]).any(0)).sum() > n // 2                     # one board's ring slots lie in different stages
    run_against_reference(g, torch_cuda, n, H, 40000, rnet, pushes, 52, boards=boards)


def test_mixed_network_4x6_4x4_td(g, torch_cuda):
    """The "4x6+4x4" preset through the Python layer, TD form (its TC accumulators are 1 GiB): the GPU against a sparse
    reference, table by table."""
    torch = torch_cuda
    n, H = 63, 3
    net = g.NTupleNet("4x6+4x4")
    assert net.mixed and net.tuples == tuple(mref.PRESET)
    sparse = {}                                                                    # compact element -> weight
    dl, rdl = g.NTupleDelay(n, depth=H, lam=0.75), dref.Delay(n, H, 49152)
    out = torch.empty(n, dtype=torch.int64, device="cuda")
    bases = mref.bases(mref.PRESET)

    def apply(mode):
        boards, Ds = dref.due_items(rdl, mode)
        for b, D in zip(boards, Ds):
            step = ref.step_of(D, 2)
            for s in (ref.symmetries(ref.plain(b)) if step else ()):
                for t, cells in enumerate(mref.PRESET):
                    e = bases[t] + ref.index(s, cells)                               # the compact element, from the definition
                    sparse[e] = ref.wrap32(sparse.get(e, 0) + step)

    for t, (after, av, bn, term) in enumerate(push_inputs(n, 6, 60)):
        push_both(torch, dl, rdl, out, after, av, bn, term, f"push {t}")
        net.delay_update(dl, 2)
        apply(dref.STEP)
    net.delay_update(dl, 2, flush=True)
    apply(dref.FLUSH)
    keys = sorted(sparse)
    assert keys[-1] >= 4 * 16 ** 6 and keys[0] < 16 ** 6                           # 6-tuple and 4-tuple tables are written
    got = net.weights[torch.as_tensor(keys, device="cuda")].cpu().numpy().astype(np.int64)
    assert np.array_equal(got, np.array([sparse[k] for k in keys], np.int64))
    assert int(torch.count_nonzero(net.weights)) == sum(1 for k in keys if sparse[k])


# ------------------------------------------------------------------------------------------- the composition oracle
def due_D(torch, dl, k, mode):
    """D of item (k, i) for every board by torch integer ops, zero where the item is not due."""
    H = dl.depth
    L = (dl.len & 0x7f).clamp(max=H)
    ended = (dl.len & 0x80) != 0
    leaving = ended | torch.full_like(ended, k == H - 1)
    due = (L > k) & (leaving != bool(mode))
    D = dl.acc[(dl.slot - k) % H].clamp(-MAXD, MAXD)
    return torch.where(due, D, torch.zeros_like(D)).contiguous()


def composed(g, torch, dl, mode, lr_shift, tuples, ks=None):
    """(TD weights, TC weights, err, mag) by the one-step kernels: per k, net.update / tc_update(phases=1) / tc_update(
    phases=2) on the slot k pushes back with D."""
    H = dl.depth
    ks = range(H) if ks is None else ks
    td, tcn = g.NTupleNet(tuples), g.NTupleNet(tuples)
    tc = g.NTupleTC(tcn)
    Ds = {k: due_D(torch, dl, k, mode) for k in ks}
    for k in ks:
        td.update(dl.hist[(dl.slot - k) % H], Ds[k], lr_shift)
    for phase in (1, 2):
        for k in ks:
            tcn.tc_update(dl.hist[(dl.slot - k) % H], Ds[k], lr_shift, tc, phase)
    return td.weights, tcn.weights, tc.err, tc.mag


def delayed(g, torch, dl, mode, lr_shift, tuples):
    td, tcn = g.NTupleNet(tuples), g.NTupleNet(tuples)
    tc = g.NTupleTC(tcn)
    td.delay_update(dl, lr_shift, flush=bool(mode))
    tcn.tc_delay_update(dl, lr_shift, tc, phases=1, flush=bool(mode))
    tcn.tc_delay_update(dl, lr_shift, tc, phases=2, flush=bool(mode))
    return td.weights, tcn.weights, tc.err, tc.mag


def test_composition_small_against_reference_too(g, torch_cuda):
    """The oracle itself, where the reference can check it: n = 257, H = 8, after nine synthetic pushes."""
    torch = torch_cuda
    n, H = 257, 8
    dl, rdl = g.NTupleDelay(n, depth=H, lam=0.75), dref.Delay(n, H, 49152)
    out = torch.empty(n, dtype=torch.int64, device="cuda")
    for after, av, bn, term in push_inputs(n, 9, 401, span=1 << 40):
        push_both(torch, dl, rdl, out, after, av, bn, term)
    for mode in (dref.STEP, dref.FLUSH):
        got, want = delayed(g, torch, dl, mode, 12, TUPLES_17x4), composed(g, torch, dl, mode, 12, TUPLES_17x4)
        rnet = ref.Net(TUPLES_17x4, 10)
        dref.delay_update(rnet, rdl, 12, mode)
        assert (rnet.weights != 0).any() and np.array_equal(want[0].cpu().numpy(), rnet.weights)
        for name, a, b in zip(("td weights", "tc weights", "err", "mag"), got, want):
            assert torch.equal(a, b), (mode, name)


def test_composition_past_the_grid_cap(g, torch_cuda):
    """n = 2^21 + 3, H = 8: 2^24 + 24 items, more than one grid covers.  Every board ended at the last push, so all of them
    are due in STEP mode; the items past the cap are k = 7 of the last 24 boards, and their D takes a step.  Then the same
    ring with no board ended: STEP applies the k = 7 plane alone and FLUSH the other seven."""
    torch = torch_cuda
    n, H, lr_shift = (1 << 21) + 3, 8, 14
    assert H * n > SEARCH_MAX_LANES and H * n - SEARCH_MAX_LANES == 24 and 7 * n + (n - 24) == SEARCH_MAX_LANES
    gen = torch.Generator(device="cuda").manual_seed(5)
    dl = g.NTupleDelay(n, depth=H, lam=0.75)
    dl.hist.copy_(torch.randint(0, 16, (H, n, 16), generator=gen, device="cuda", dtype=torch.uint8))
    dl.acc.copy_(torch.randint(-(1 << 43), 1 << 43, (H, n), generator=gen, device="cuda", dtype=torch.int64))
    dl.acc[torch.rand((H, n), generator=gen, device="cuda") < 0.875] = 0
    dl.slot = 5
    tail = torch.arange(1, 25, device="cuda", dtype=torch.int64) << 30
    dl.acc[(dl.slot - 7) % H, -24:] = torch.where(torch.arange(24, device="cuda") % 2 == 0, tail, -tail)
    assert int(dl.acc.abs().max()) > MAXD and all(ref.step_of(tcref.clamp_delta(d), lr_shift) != 0 for d in dl.acc[(dl.slot - 7) % H, -24:].tolist())
    dl.len.fill_(0x88)
    got = delayed(g, torch, dl, dref.STEP, lr_shift, TUPLES_17x4)
    want = composed(g, torch, dl, dref.STEP, lr_shift, TUPLES_17x4)
    for name, a, b in zip(("td weights", "tc weights", "err", "mag"), got, want):
        assert torch.equal(a, b), name
    assert not delayed(g, torch, dl, dref.FLUSH, lr_shift, TUPLES_17x4)[0].any()   # ended boards have nothing to flush
    # without the 24 items past the cap the tables would differ: their contribution alone is not zero
    only = torch.zeros(n, dtype=torch.int64, device="cuda")
    only[-24:] = dl.acc[(dl.slot - 7) % H, -24:]
    alone = g.NTupleNet(TUPLES_17x4)
    alone.update(dl.hist[(dl.slot - 7) % H], only, lr_shift)
    assert bool(alone.weights.any())
    # no termination: STEP is the k = 7 plane alone, FLUSH the other seven
    dl.len.fill_(8)
    got = delayed(g, torch, dl, dref.STEP, lr_shift, TUPLES_17x4)
    want = composed(g, torch, dl, dref.STEP, lr_shift, TUPLES_17x4, ks=(7,))
    for name, a, b in zip(("td weights", "tc weights", "err", "mag"), got, want):
        assert torch.equal(a, b), "k = 7 alone: " + name
    got = delayed(g, torch, dl, dref.FLUSH, lr_shift, TUPLES_17x4)
    want = composed(g, torch, dl, dref.FLUSH, lr_shift, TUPLES_17x4, ks=range(7))
    for name, a, b in zip(("td weights", "tc weights", "err", "mag"), got, want):
        assert torch.equal(a, b), "flush: " + name


def test_ring_above_4_gib(g, torch_cuda):
    """n = 2^25 + 3, H = 8, one 4-tuple: hist is 4 GiB + 384 bytes, acc 2 GiB + 192.  The push goes into slot 7, whose last 24
    boards lie at byte offsets above 2^32 in hist, and only those 24 end: a STEP update is due for them alone, in that slot."""
    torch = torch_cuda
    n, H, lr_shift = (1 << 25) + 3, 8, 3
    tuples = ((0, 1, 4, 5),)
    dl = g.NTupleDelay(n, depth=H, lam=1.0)
    assert dl.hist.numel() > 1 << 32 and (7 * n + n - 24) * 16 >= 1 << 32 and dl.acc.numel() * 8 > 1 << 31
    ends = np.r_[0:5, n - 24:n]
    after = torch.zeros((n, 16), dtype=torch.uint8, device="cuda")
    after[dev(torch, ends)] = dev(torch, random_boards(29, 21))
    values = torch.zeros(n, dtype=torch.int64, device="cuda")
    best = torch.zeros(n, dtype=torch.int64, device="cuda")
    values[dev(torch, ends)] = dev(torch, (np.arange(29, dtype=np.int64) * 2 + 5) * np.where(np.arange(29) % 2, -1, 1) << 20)
    values[n - 1], values[n - 2] = -(MAXD + 12345), 1 << 62                        # both clamp in the accumulator
    term = torch.zeros(n, dtype=torch.uint8, device="cuda")
    term[-24:] = 0xff
    delta = torch.empty(n, dtype=torch.int64, device="cuda")
    dl.slot = 6
    dl.push(after, values, best, term, delta)
    assert dl.slot == 7 and torch.equal(delta, -values) and int(torch.count_nonzero(delta)) == 29
    assert torch.equal(dl.acc[7], delta.clamp(-MAXD, MAXD)) and not dl.acc[:7].any()
    assert torch.equal(dl.hist[7, :5], after[:5]) and torch.equal(dl.hist[7, -24:], after[-24:])
    assert not dl.hist[:7].any() and int(torch.count_nonzero(dl.hist[7])) == int(torch.count_nonzero(after))
    assert int((dl.len == 1).sum()) == n - 24 and bool((dl.len[-24:] == 0x81).all())
    snapshot = dl.acc[7].clone()
    got = delayed(g, torch, dl, dref.STEP, lr_shift, tuples)
    assert torch.equal(dl.acc[7], snapshot)
    # the 24 boards against the reference and against the one-step kernels
    D = delta[-24:].clamp(-MAXD, MAXD).contiguous()
    rnet = ref.Net(tuples, 10)
    ref.update(rnet, after[-24:].cpu().numpy(), D.cpu().numpy(), lr_shift)
    assert (rnet.weights != 0).any() and np.array_equal(got[0].cpu().numpy(), rnet.weights)
    tcn = g.NTupleNet(tuples)
    tc = g.NTupleTC(tcn)
    tcn.tc_update(after[-24:].contiguous(), D, lr_shift, tc)
    for name, a, b in zip(("tc weights", "err", "mag"), got[1:], (tcn.weights, tc.err, tc.mag)):
        assert torch.equal(a, b), name
    # the flush is due for every other board, k = 0 in slot 7: the first five have an error
    flushed = g.NTupleNet(tuples)
    flushed.delay_update(dl, lr_shift, flush=True)
    rnet = ref.Net(tuples, 10)
    ref.update(rnet, after[:5].cpu().numpy(), delta[:5].cpu().numpy(), lr_shift)
    assert (rnet.weights != 0).any() and np.array_equal(flushed.weights.cpu().numpy(), rnet.weights)


# --------------------------------------------------------------------------------------------------- engine level
ENGINE = dict(n=64, steps=300, seed=42, lr_shift=5)


def engine(g, n=None, **kw):
    eng = g.Batched2048(n or ENGINE["n"], seed=ENGINE["seed"], **kw)
    eng.reset()
    return eng


def test_delayed_tdl_train_at_h_1_is_train(g, torch_cuda):
    torch = torch_cuda
    want, eng = g.NTupleNet("17x4"), engine(g)
    try:
        g.train(eng, want, ENGINE["steps"], ENGINE["lr_shift"])
        episodes = eng.episode_stats()["episodes"]
    finally:
        eng.close()
    assert episodes >= 1, f"no game finished in {ENGINE['steps']} steps: raise the step count"
    net, eng = g.NTupleNet("17x4"), engine(g)
    try:
        dl = g.NTupleDelay(ENGINE["n"], depth=1, lam=0.5)
        assert g.delayed_tdl_train(eng, net, dl, ENGINE["steps"], ENGINE["lr_shift"]) is net
        torch.cuda.synchronize()
        assert torch.equal(net.weights, want.weights) and bool(want.weights.any()) and eng.episode_stats()["episodes"] == episodes
        assert not dl.len.any()
    finally:
        eng.close()


def test_delayed_tcl_train_at_h_1_is_tc_train(g, torch_cuda):
    torch = torch_cuda
    want, eng = g.NTupleNet("17x4"), engine(g)
    want_tc = g.NTupleTC(want)
    try:
        g.tc_train(eng, want, want_tc, ENGINE["steps"], ENGINE["lr_shift"])
        episodes = eng.episode_stats()["episodes"]
    finally:
        eng.close()
    assert episodes >= 1, f"no game finished in {ENGINE['steps']} steps: raise the step count"
    net, eng = g.NTupleNet("17x4"), engine(g)
    tc = g.NTupleTC(net)
    try:
        dl = g.NTupleDelay(ENGINE["n"], depth=1, lam=0.5)
        assert g.delayed_tcl_train(eng, net, tc, dl, ENGINE["steps"], ENGINE["lr_shift"]) is net
        torch.cuda.synchronize()
        assert torch.equal(net.weights, want.weights) and torch.equal(tc.err, want_tc.err) and torch.equal(tc.mag, want_tc.mag)
        assert bool(want_tc.err.any()) and eng.episode_stats()["episodes"] == episodes and not dl.len.any()
    finally:
        eng.close()


@pytest.mark.parametrize("form", ["td", "tc"])
def test_delayed_train_equals_the_reference_replaying_the_run(g, torch_cuda, form):
    """H = 4, lambda = 0.5, 64 boards, 200 steps: the afterstates, values and flags of every step are recorded from the GPU
    run (the ``*_step`` functions and the flush that ``*_train`` ends with); the reference pushes and updates them on the CPU.
    After the flush nothing is pending: a reset ring flushes nothing, and ``*_train`` leaves ``len`` zero."""
    from gym2048_amd.ntuple import delayed_tcl_step, delayed_tdl_step, td_work
    torch = torch_cuda
    H, lam, steps, shift = 4, 32768, 200, ENGINE["lr_shift"]
    net, eng = g.NTupleNet("17x4"), engine(g)
    tc = g.NTupleTC(net) if form == "tc" else None
    try:
        dl, work, rec = g.NTupleDelay(ENGINE["n"], depth=H, lam=0.5), td_work(eng), []
        for _ in range(steps):
            if tc is None:
                delayed_tdl_step(eng, net, dl, shift, work)
            else:
                delayed_tcl_step(eng, net, tc, dl, shift, work)
            rec.append([t.cpu().numpy() for t in (work.before.after, work.before.after_value, work.after.best, eng.terminated, work.delta)])
        episodes = eng.episode_stats()["episodes"]
        pending = net.weights.clone()
        if tc is None:
            net.delay_update(dl, shift, flush=True)
        else:
            net.tc_delay_update(dl, shift, tc, flush=True)
        assert not torch.equal(net.weights, pending)                              # the flush had errors to apply
        got_ring = dl.slot, dl.len.cpu().numpy(), dl.hist.cpu().numpy(), dl.acc.cpu().numpy()
        dl.reset()
        flushed = net.weights.clone()
        if tc is None:
            net.delay_update(dl, shift, flush=True)
        else:
            net.tc_delay_update(dl, shift, tc, flush=True)
        assert torch.equal(net.weights, flushed) and not dl.len.any()             # a second flush changes nothing
        got = tables(net, tc)
    finally:
        eng.close()
    assert episodes >= 1, f"no game finished in {steps} steps: raise the step count"
    rnet, rdl = mref.mixed_net(TUPLES_17x4), dref.Delay(ENGINE["n"], H, lam)
    rtc = mref.tc_of(rnet)
    terms = 0
    for after, av, bn, term, delta in rec:
        assert np.array_equal(dref.push(rdl, after, av, bn, term), delta)
        terms += int(np.count_nonzero(term))
        for mode in (dref.STEP,):
            if tc is None:
                dref.delay_update(rnet, rdl, shift, mode)
            else:
                dref.tc_delay_update(rnet, rtc, rdl, shift, 3, mode)
    assert terms == episodes
    assert got_ring[0] == rdl.slot and all(np.array_equal(a, b) for a, b in zip(got_ring[1:], (rdl.len, rdl.hist, rdl.acc_i64())))
    if tc is None:
        dref.delay_update(rnet, rdl, shift, dref.FLUSH)
    else:
        dref.tc_delay_update(rnet, rtc, rdl, shift, 3, dref.FLUSH)
    assert_tables_equal(got, want_tables(rnet, None if tc is None else rtc))


@pytest.mark.parametrize("form", ["td", "tc"])
def test_train_flushes_and_resets(g, torch_cuda, form):
    """``*_train`` is the steps, the flush and the reset: equal to doing them by hand, ``len`` all zero afterwards, and a
    flush after it changes nothing."""
    from gym2048_amd.ntuple import delayed_tcl_step, delayed_tdl_step, td_work
    torch = torch_cuda
    steps, shift, results = 120, ENGINE["lr_shift"], []
    for by_hand in (False, True):
        net, eng = g.NTupleNet("17x4"), engine(g)
        tc = g.NTupleTC(net)
        dl = g.NTupleDelay(ENGINE["n"], depth=4, lam=0.5)
        try:
            if not by_hand:
                (g.delayed_tdl_train(eng, net, dl, steps, shift) if form == "td" else g.delayed_tcl_train(eng, net, tc, dl, steps, shift))
                assert not dl.len.any() and bool(dl.acc.any())
                before = tables(net, tc)
                (net.delay_update(dl, shift, flush=True) if form == "td" else net.tc_delay_update(dl, shift, tc, flush=True))
                assert_tables_equal(tables(net, tc), before)
            else:
                work = td_work(eng)
                for _ in range(steps):
                    (delayed_tdl_step(eng, net, dl, shift, work) if form == "td" else delayed_tcl_step(eng, net, tc, dl, shift, work))
                assert bool((dl.len & 0x7f).any())
                (net.delay_update(dl, shift, flush=True) if form == "td" else net.tc_delay_update(dl, shift, tc, flush=True))
            torch.cuda.synchronize()
            results.append(tables(net, tc))
        finally:
            eng.close()
    assert_tables_equal(results[0], results[1])
    assert results[0][0].any() and (form == "td" or results[0][1].any())


@pytest.mark.parametrize("form", ["td", "tc"])
def test_two_shards_with_their_own_delays_equal_the_unsharded_run(g, torch_cuda, form):
    """Consequence 4: push everywhere, then update everywhere; for TC, W everywhere, then A everywhere; the flush likewise."""
    from gym2048_amd.ntuple import delayed_evaluate, td_work
    torch = torch_cuda
    n, cut, H, lam, shift, steps = ENGINE["n"], 24, 4, 0.5, ENGINE["lr_shift"], 150
    whole, eng = g.NTupleNet("17x4"), engine(g)
    whole_tc = g.NTupleTC(whole)
    try:
        if form == "td":
            g.delayed_tdl_train(eng, whole, g.NTupleDelay(n, depth=H, lam=lam), steps, shift)
        else:
            g.delayed_tcl_train(eng, whole, whole_tc, g.NTupleDelay(n, depth=H, lam=lam), steps, shift)
        boards = eng.get_boards()
    finally:
        eng.close()
    assert bool(whole.weights.any())
    net = g.NTupleNet("17x4")
    tc = g.NTupleTC(net)
    a, b = g.Batched2048(cut, seed=ENGINE["seed"]), g.Batched2048(n - cut, seed=ENGINE["seed"], board_offset=cut)
    try:
        shards = [(e, g.NTupleDelay(e.n_envs, depth=H, lam=lam), td_work(e)) for e in (a, b)]
        for e in (a, b):
            e.reset()

        def update(flush):
            if form == "tc":
                for phase in (1, 2):
                    for e, dl, w in shards:
                        net.tc_delay_update(dl, shift, tc, phases=phase, flush=flush)
            else:
                for e, dl, w in shards:
                    net.delay_update(dl, shift, flush=flush)

        for _ in range(steps):
            for e, dl, w in shards:
                delayed_evaluate(e, net, dl, w)
            update(False)
        update(True)
        torch.cuda.synchronize()
        assert_tables_equal(tables(net, tc), tables(whole, whole_tc))
        assert np.array_equal(np.concatenate([a.get_boards(), b.get_boards()]), boards)
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------------------------------------------- the Python layer
def test_state_dict_round_trip_in_the_middle_of_a_run(g, torch_cuda):
    """Six pushes with updates, a snapshot, six more and the flush -- against a fresh ring and network that load the snapshot
    and run the last six: the continued run equals the uninterrupted one."""
    torch = torch_cuda
    n, H, shift = 50, 4, 9
    inputs = [[dev(torch, x) for x in row] for row in push_inputs(n, 12, 501)]
    rnet = ref_net(TUPLES_17x4, 502)
    rtc = random_tc(rnet, 503)
    net, tc = device_state(g, torch, rnet, rtc)
    dl = g.NTupleDelay(n, depth=H, lam=0.5)
    out = torch.empty(n, dtype=torch.int64, device="cuda")

    def run(net, tc, dl, rows):
        for row in rows:
            dl.push(*row, out)
            net.tc_delay_update(dl, shift, tc)

    run(net, tc, dl, inputs[:6])
    state, saved = dl.state_dict(), (net.state_dict(), tc.state_dict())
    assert set(state) == {"depth", "lam_q16", "slot", "hist", "len", "acc"} and state["slot"] == dl.slot == 5 % H
    assert state["acc"].data_ptr() != dl.acc.data_ptr() and bool(state["acc"].any()) and bool(state["len"].any())
    run(net, tc, dl, inputs[6:])
    net.tc_delay_update(dl, shift, tc, flush=True)
    net2, tc2 = device_state(g, torch, rnet, rtc)
    net2.load_state_dict(saved[0])
    tc2.load_state_dict(saved[1])
    dl2 = g.NTupleDelay(n, depth=H, lam=0.5)
    ptrs = dl2.hist.data_ptr(), dl2.len.data_ptr(), dl2.acc.data_ptr()
    dl2.load_state_dict({k: v.cpu() if isinstance(v, torch.Tensor) else v for k, v in state.items()})
    assert ptrs == (dl2.hist.data_ptr(), dl2.len.data_ptr(), dl2.acc.data_ptr()) and dl2.slot == state["slot"]
    run(net2, tc2, dl2, inputs[6:])
    net2.tc_delay_update(dl2, shift, tc2, flush=True)
    assert_tables_equal(tables(net2, tc2), tables(net, tc))
    assert torch.equal(dl2.acc, dl.acc) and torch.equal(dl2.hist, dl.hist) and torch.equal(dl2.len, dl.len) and dl2.slot == dl.slot
    for bad, match in ((dict(state, depth=2), "another depth or lam"), (dict(state, lam_q16=1), "another depth or lam"),
                       (dict(state, acc=state["acc"][:, :10]), "acc must be int64"), (dict(state, len=state["len"].to(torch.int32)), "len must be uint8"),
                       (dict(state, slot=4), "slot")):
        with pytest.raises(ValueError, match=match):
            dl2.load_state_dict(bad)


def test_bad_arguments_are_refused_and_touch_nothing(g, torch_cuda):
    torch = torch_cuda
    from gym2048_amd import _lib
    lib = _lib.load()
    n = 16
    rnet = ref_net(TUPLES_17x4, 121)
    net, tc = device_state(g, torch, rnet, random_tc(rnet, 122))
    dl = g.NTupleDelay(n, depth=4, lam=0.5)
    out = torch.zeros(n, dtype=torch.int64, device="cuda")
    for row in push_inputs(n, 5, 601):
        dl.push(*[dev(torch, x) for x in row], out)
    dl.len.fill_(0x84)                                                           # every item is due: a call that ran would show
    before = tables(net, tc), dl.hist.clone(), dl.len.clone(), dl.acc.clone(), dl.slot, out.clone()
    d64 = torch.full((n,), 1 << 20, dtype=torch.int64, device="cuda")
    after = dev(torch, random_boards(n, 123))
    term = torch.zeros(n, dtype=torch.uint8, device="cuda")
    other_net = g.NTupleNet("17x4")
    elsewhere = g.NTupleDelay(n)
    elsewhere.device = torch.device("cuda:1")           # a delay that says it lives on another device
    for call, match in (
            (lambda: net.delay_update(dl, 41), "lr_shift"), (lambda: net.delay_update(dl, -1), "lr_shift"),
            (lambda: net.delay_update(None, 3), "delay must be"), (lambda: net.delay_update(g.NTupleTrace(n), 3), "delay must be"),
            (lambda: net.delay_update(elsewhere, 3), "weights are on"), (lambda: net.delay_update(dl, 3, flush=2), "flush"),
            (lambda: net.tc_delay_update(elsewhere, 3, tc), "weights are on"), (lambda: net.tc_delay_update(dl, 3, tc, phases=0), "phases"),
            (lambda: net.tc_delay_update(dl, 3, tc, phases=4), "phases"), (lambda: net.tc_delay_update(dl, 3, None), "tc must be"),
            (lambda: net.tc_delay_update(dl, 3, g.NTupleTC(other_net)), "tc must be"), (lambda: net.tc_delay_update(dl, 3, tc, flush=7), "flush"),
            (lambda: dl.push(after[:, :15], d64, d64, term, out), "after must be"),
            (lambda: dl.push(after, d64.to(torch.int32), d64, term, out), "after_value must be"),
            (lambda: dl.push(after, d64, d64[:-1], term, out), "best_next must be"),
            (lambda: dl.push(after, d64, d64, term.to(torch.int64), out), "terminated must be"),
            (lambda: dl.push(after, d64, d64, term, out.cpu()), "out must be"),
            (lambda: g.NTupleDelay(0), "n"), (lambda: g.NTupleDelay(4, depth=0), "depth"), (lambda: g.NTupleDelay(4, depth=9), "depth"),
            (lambda: g.NTupleDelay(4, lam=1.5), "lam"), (lambda: g.NTupleDelay(4, lam="x"), "lam")):
        with pytest.raises(ValueError, match=match):
            call()
    # the library refuses what gets past Python: a slot, a mode, a misaligned or missing accumulator array
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)           # noqa: E731
    odd = _lib.NTupleDelayC(4, 32768, dl.hist.data_ptr(), dl.len.data_ptr(), dl.acc.data_ptr() + 4)
    none = _lib.NTupleDelayC(4, 32768, dl.hist.data_ptr(), dl.len.data_ptr(), None)
    for call, message in (
            (lambda: lib.g2048_ntuple_delay_update(n, 3, 0, C.byref(net._c), C.byref(dl._c), 4, st()), b"slot=4"),
            (lambda: lib.g2048_ntuple_delay_update(n, 3, 2, C.byref(net._c), C.byref(dl._c), 0, st()), b"mode=2"),
            (lambda: lib.g2048_ntuple_tc_delay_update(n, 3, 3, 2, C.byref(net._c), C.byref(tc._c), C.byref(dl._c), 0, st()), b"mode=2"),
            (lambda: lib.g2048_ntuple_tc_delay_update(n, 3, 4, 0, C.byref(net._c), C.byref(tc._c), C.byref(dl._c), 0, st()), b"phases=4"),
            (lambda: lib.g2048_ntuple_delay_update(n, 3, 0, C.byref(net._c), C.byref(odd), 0, st()), b"delay acc needs 8 bytes"),
            (lambda: lib.g2048_ntuple_delay_update(n, 3, 0, C.byref(net._c), C.byref(none), 0, st()), b"delay acc is NULL"),
            (lambda: lib.g2048_ntuple_delay_push(after.data_ptr(), d64.data_ptr(), d64.data_ptr(), term.data_ptr(), n, C.byref(odd), 0,
                                         out.data_ptr(), st()), b"delay acc needs 8 bytes"),
            (lambda: lib.g2048_ntuple_delay_push(after.data_ptr(), d64.data_ptr(), d64.data_ptr(), term.data_ptr(), n, C.byref(dl._c), 4,
                                         out.data_ptr(), st()), b"slot=4")):
        assert call() == -1 and message in lib.g2048_last_error()
    torch.cuda.synchronize()
    assert_tables_equal(tables(net, tc), before[0])
    assert torch.equal(dl.hist, before[1]) and torch.equal(dl.len, before[2]) and torch.equal(dl.acc, before[3])
    assert dl.slot == before[4] and torch.equal(out, before[5])
    assert lib.g2048_abi_version() == _lib.ABI_VERSION == 16
