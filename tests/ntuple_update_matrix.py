"""Shared by tests/test_gpu_ntuple_update_matrix.py, tests/test_ntuple_update_matrix_cpu.py and tests/test_gpu_ntuple_delay.py:
the cases that take every instantiation of the three n-tuple update kernels through the pure-Python references, computed once,
and the replay of a delay run on the device.  A plain module, like ntuple_deep_helpers.

Families (``family_net``), as ntuple_deep_helpers.FAMILIES -- 23 networks, every one an ntuple_mixed_ref.mixed_net on the padded
array (``thr = ()`` for the uniform family), so one reference path and one device constructor serve them all:
  uniform  TUPLES_8x4[:T], T = 1..8, S = 1
  staged   TUPLES_8x4[:T] on THR_3 (S = 3), T = 1..8
  mixed    ntuple_mixed_ref.MIX_8[:T] on THR_3 (S = 3), T = 2..8
Weights are full-range random int32 and the accumulators ntuple_mixed_helpers.random_tc's; network T has the first T tables (of
every stage) of the family's network 8, weights and accumulators alike.

Sources (``board_case``, ``trace_case``, ``delay_case``): 65 boards -- one workgroup, a full wave and one lane --
  board  small_boards and edge_deltas, lr_shift 3
  trace  H = 4, lam_q16 = 49152, 7 pushes of small_boards through ntuple_trace_ref.push, trace_deltas, lr_shift 3
  delay  the same ring geometry and boards, push_inputs(span = 2^40) with a few values replaced so that accumulators of 0 and of
         a few units exist, lr_shift 10; a STEP update after every push and one FLUSH
The expected tables after every call are kept as their difference from the tables before the first one (``Expected``): an
update of 65 boards writes a few thousand of the up to 1.5 million entries.

``assert_conditions`` shows, from the references and the inputs alone, what a case must reach for a wrong kernel not to pass.
"""
import types

import numpy as np

import ntuple_delay_ref as dref
import ntuple_mixed_ref as mref
import ntuple_ref as ref
import ntuple_staged_ref as sref
import ntuple_tc_ref as tcref
import ntuple_trace_ref as tref
from ntuple_deep_helpers import FAMILIES
from ntuple_helpers import TUPLES_8x4
from ntuple_mixed_helpers import THR_3, random_tc, want_tables
from ntuple_staged_helpers import small_boards
from ntuple_tc_helpers import assert_tables_equal, edge_deltas
from ntuple_trace_helpers import push_inputs, trace_deltas

CASES = [(family, T) for family, counts in FAMILIES.items() for T in counts]
SOURCES = ("board", "trace", "delay")
SHAPE = {"uniform": (False, 1), "staged": (False, 3), "mixed": (True, 3)}        # (net.mixed, net.n_stages) on the device
KIND = {"uniform": 0, "staged": 1, "mixed": 2}                                    # the shape type of the host builds
N, H, LAM, PUSHES = 65, 4, 49152, 7
LR_SHIFT, DELAY_LR_SHIFT = 3, 10
MAXD = tcref.MAX_DELTA
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def case_id(case):
    return f"{case[0]}-{case[1]}"


# ------------------------------------------------------------------------------------------------ networks
def ref_net(tuples, seed, thr=()):
    """The reference network (a StagedNet on the padded array, S = len(thr) + 1): full-range random int32 everywhere."""
    return mref.mixed_net(tuples, thr, 10, mref.random_flat(tuples, seed, len(thr) + 1))


def family_tuples(family, T=8):
    return tuple((mref.MIX_8 if family == "mixed" else TUPLES_8x4)[:T])


def family_thr(family):
    return () if family == "uniform" else THR_3


def _family_flat(family):
    """(weights, err, mag) of the family's network 8, compact [S, W] int64.  (A quarter of random_tc's entries have err = 0, a rate
    of 0: in a stage that reaches two or three entries of a one-cell table the TC weights of that table may not move at all.
    With these seeds they do in every table of every stage and source; assert_conditions shows it from the reference.)"""
    def make():
        seed = 61 + sorted(FAMILIES).index(family)
        net = ref_net(family_tuples(family), seed, family_thr(family))
        return (mref.flat_of(net),) + mref.tc_flat(random_tc(net, seed + 11), net)
    return cached(("flat", family), make)


def family_net(family, T):
    """(network, accumulators) T of a family: fresh reference objects, the caller's to modify."""
    assert T in FAMILIES[family] or (family, T) == ("mixed", 1)        # ("mixed", 1): the neighbour of ("mixed", 2) only
    tuples, (w, err, mag) = family_tuples(family, T), _family_flat(family)
    W = mref.n_weights(tuples)                                           # the tables lie back to back
    net = mref.mixed_net(tuples, family_thr(family), 10, w[:, :W])
    return net, mref.tc_of(net, err[:, :W], mag[:, :W])


def base_tables(family, T):
    """(weights, err, mag) before any call: compact flat int64, as want_tables gives them."""
    return want_tables(*family_net(family, T))


class Expected:
    """Tables after a call (a tuple of flat arrays), kept as the entries that differ from the ``base`` tables."""

    def __init__(self, base, now):
        self.idx = [np.nonzero(b != a)[0] for b, a in zip(base, now)]
        self.val = [a[i].copy() for a, i in zip(now, self.idx)]

    def on(self, base):
        """The tables in full: fresh copies of ``base`` with the kept entries written."""
        out = tuple(b.copy() for b in base)
        for o, i, v in zip(out, self.idx, self.val):
            o[i] = v
        return out


def tables_hit(idx, tuples, S):
    """{(stage, t)}: the tables that the compact flat elements ``idx`` lie in."""
    W, bases = mref.n_weights(tuples), np.array(mref.bases(tuples))
    return set(zip((idx // W).tolist(), (np.searchsorted(bases, idx % W, side="right") - 1).tolist()))


def every_table(tuples, S):
    return {(s, t) for s in range(S) for t in range(len(tuples))}


def hist_span(tr, thr):
    """Boards whose valid ring slots lie in at least two stages (as "hist_span" of ntuple_staged_ref's trace)."""
    count = 0
    for i in range(tr.n):
        L = min(int(tr.len[i]) & 0x7f, tr.depth)
        count += len({sref.stage(ref.plain(tr.hist[(tr.slot + tr.depth - k) % tr.depth, i]), thr) for k in range(L)}) > 1
    return count


def pool():
    """[PUSHES, N, 16]: the boards of every source; the board source takes the first batch."""
    return cached("pool", lambda: small_boards(N * PUSHES, 50).reshape(PUSHES, N, 16))


# ------------------------------------------------------------------------------------------------ board and trace items
def _one_call(family, T, td_update, tc_update):
    """(Expected of the TD update, Expected of the TC update) of a case; the updates take (net[, tc]) and work in place."""
    base = base_tables(family, T)
    net, _ = family_net(family, T)
    td_update(net)
    td = Expected(base[:1], want_tables(net))
    net, tc = family_net(family, T)
    tc_update(net, tc)
    return td, Expected(base, want_tables(net, tc))


def board_case(family, T):
    """boards, deltas, lr_shift, the Expected tables ``td`` and ``tc`` (phases W and A), ``trace`` of the staged reference."""
    def make():
        boards, deltas, trace = pool()[0], edge_deltas(N, 9), {}
        td, tc = _one_call(family, T, lambda net: sref.update(net, boards, deltas, LR_SHIFT, trace),
                           lambda net, tc: sref.tc_update(net, tc, boards, deltas, LR_SHIFT, 3))
        return types.SimpleNamespace(boards=boards, deltas=deltas, lr_shift=LR_SHIFT, td=td, tc=tc, trace=trace)
    return cached(("board", family, T), make)


def pushed_ring():
    """The reference trace after the PUSHES pushes (not to be modified), and the inputs of the pushes with the boards of pool()."""
    def make():
        tr, rows = tref.Trace(N, H, LAM), []
        for t, (_, av, bn, term) in enumerate(push_inputs(N, PUSHES, 11, span=1 << 40)):
            rows.append((pool()[t], av, bn, term))
            tref.push(tr, *rows[-1])
        return tr, rows
    return cached("ring", make)


def trace_case(family, T):
    """tr (the reference trace), deltas, lr_shift, ``td``, ``tc`` and ``trace`` as board_case."""
    def make():
        tr, deltas, trace = pushed_ring()[0], trace_deltas(N, 12), {}
        td, tc = _one_call(family, T, lambda net: sref.trace_update(net, tr, deltas, LR_SHIFT, trace),
                           lambda net, tc: sref.tc_trace_update(net, tc, tr, deltas, LR_SHIFT, 3))
        return types.SimpleNamespace(tr=tr, deltas=deltas, lr_shift=LR_SHIFT, td=td, tc=tc, trace=trace)
    return cached(("trace", family, T), make)


# ------------------------------------------------------------------------------------------------ the delay run
ALTERNATE = lambda t: t is not None and t % 2 == 1      # noqa: E731  TC as one call on even pushes and the flush, as two on odd ones
ONE_CALL = lambda t: False                              # noqa: E731
TWO_CALLS = lambda t: True                              # noqa: E731


def delay_inputs():
    """The pushes of the delay source: pushed_ring's, with boards 3, 10 and 17 (which end at different pushes) given equal
    values -- a delta of 0 wherever the episode goes on -- and boards 4 and 11 a delta of 5 or -7: accumulators that stay 0 or a
    few units, whose step at lr_shift 10 is 0 while their phase A is not."""
    def make():
        rows = []
        for after, av, bn, term in pushed_ring()[1]:
            av, bn = av.copy(), bn.copy()
            av[[3, 10, 17]], bn[[3, 10, 17]] = 0, 0
            av[[4, 11]], bn[[4, 11]] = 0, (5, -7)
            rows.append((after, av, bn, term))
        return rows
    return cached("delay inputs", make)


def delay_reference(n, depth, lam, state, inputs, lr_shift=10, tc_form=True):
    """The reference over ``inputs`` (a list of (after, after_value, best_next, terminated)): each push is followed by the TD
    update on one network and by TC W + A on another, then the FLUSH.  ``state()`` gives fresh (network, accumulators).
    Returns the calls -- per call the push (its inputs, delta and the ring after it; None for the flush), the mode, the Expected
    tables ``td`` and ``tc``, the due items and ``span``, the boards whose valid slots lie in two stages -- and the number of
    afterstates applied by STEP updates and by the FLUSH."""
    rdl = dref.Delay(n, depth, lam)
    want_td, rtc = state()
    want_tcn, want_tc = state() if tc_form else (None, None)
    base = want_tables(want_td, rtc if tc_form else None)
    calls, applied = [], {dref.STEP: 0, dref.FLUSH: 0}

    def update(t, mode, push, where):
        boards, Ds = dref.due_items(rdl, mode)
        applied[mode] += len(Ds)
        dref.delay_update(want_td, rdl, lr_shift, mode)
        td, tc = Expected(base[:1], want_tables(want_td)), None
        if tc_form:
            dref.tc_delay_update(want_tcn, want_tc, rdl, lr_shift, 3, mode)
            tc = Expected(base, want_tables(want_tcn, want_tc))
        calls.append(types.SimpleNamespace(t=t, mode=mode, push=push, where=where, td=td, tc=tc, boards=boards, Ds=Ds,
                                           span=hist_span(rdl, want_td.thr), ring=rdl.copy()))

    for t, (after, av, bn, term) in enumerate(inputs):
        delta = dref.push(rdl, after, av, bn, term)
        update(t, dref.STEP, types.SimpleNamespace(after=after, after_value=av, best_next=bn, terminated=term, delta=delta), f"push {t}")
    update(None, dref.FLUSH, None, "flush")
    assert applied[dref.STEP] + applied[dref.FLUSH] == n * len(inputs)             # every pushed afterstate exactly once
    return types.SimpleNamespace(n=n, depth=depth, lam=lam, lr_shift=lr_shift, tc_form=tc_form, state=state, calls=calls,
                                 applied=applied, ring=rdl)


def delay_case(family, T):
    return cached(("delay", family, T), lambda: delay_reference(N, H, LAM, lambda: family_net(family, T), delay_inputs(), DELAY_LR_SHIFT))


def case_of(family, T, source):
    return {"board": board_case, "trace": trace_case, "delay": delay_case}[source](family, T)


def final_tables(family, T, source):
    """(Expected TD tables, Expected TC tables) after the last call of a case."""
    case = case_of(family, T, source)
    return (case.calls[-1].td, case.calls[-1].tc) if source == "delay" else (case.td, case.tc)


# ------------------------------------------------------------------------------------------------ what a case reaches
def _stages_of(boards, thr):
    return set(sref.stage_batch(boards, thr).tolist())


def assert_conditions(family, T, source):
    """What the references and the inputs say about a case -- nothing here has seen the code under test."""
    case, tuples, thr = case_of(family, T, source), family_tuples(family, T), family_thr(family)
    S, staged = len(thr) + 1, family != "uniform"
    td, tc = final_tables(family, T, source)
    base = base_tables(family, T)
    # every table of every stage is written, by every kernel: the instantiation of T - 1 leaves table T - 1 as it was, the
    # uniform shape every stage but the first
    for name, idx in (("td weights", td.idx[0]), ("tc weights", tc.idx[0]), ("err", tc.idx[1]), ("mag", tc.idx[2])):
        assert tables_hit(idx, tuples, S) == every_table(tuples, S), f"inputs: {name} does not change in every table of every stage"
    # a TC entry point that reached the TD kernel would give the TD weights
    assert (td.on(base[:1])[0] != tc.on(base)[0]).any(), "inputs: the TC weights are the TD weights"
    if T > 1:
        # the tables the instantiation of T - 1 would leave: network T - 1's (its tables are this network's first T - 1, and
        # every entry moves by its own table's steps alone) and table T - 1 untouched
        Wn, Wp = mref.n_weights(tuples), mref.n_weights(tuples[:-1])
        for mine, theirs, b in zip((td, tc), final_tables(family, T - 1, source), (base[:1], base)):
            prev, want = theirs.on(base_tables(family, T - 1)[:len(b)]), mine.on(b)
            for p, w, o in zip(prev, want, b):
                left = o.copy().reshape(S, Wn)
                left[:, :Wp] = p.reshape(S, Wp)
                assert (left.reshape(-1) != w).any(), "inputs: the neighbouring instantiation would leave the same tables"
    if source == "board":
        boards, deltas, lr = [case.boards], case.deltas, case.lr_shift
        Ds = [tcref.clamp_delta(int(d)) for d in deltas]
        clamped = any(abs(int(d)) > MAXD for d in deltas)
    elif source == "trace":
        tr = case.tr
        boards, deltas, lr = [pool()[-H:]], case.deltas, case.lr_shift
        Ds = [tref.d_k(int(d), tr.lam, k) for d, ln in zip(deltas, tr.len) for k in range(min(int(ln) & 0x7f, H))]
        clamped = any(abs(int(d)) > MAXD for d in deltas)
        rings = [tr]
        spans = [case.trace.get("hist_span", 0)]
        assert not staged or set(case.trace["stage"]) == {0, 1, 2}, "inputs: the items lie in all three stages"
    else:
        boards, lr = [c.boards for c in case.calls], case.lr_shift
        Ds = [D for c in case.calls for D in c.Ds]
        clamped = any(abs(int(d)) > MAXD for c in case.calls if c.push for d in c.push.delta)
        rings = [c.ring for c in case.calls]
        spans = [c.span for c in case.calls]
        assert case.applied[dref.STEP] > 0 and case.applied[dref.FLUSH] > 0, "inputs: both modes apply afterstates"
        assert case.applied[dref.STEP] + case.applied[dref.FLUSH] == N * PUSHES
        assert any(D != 0 and ref.step_of(D, lr) == 0 for D in Ds), "inputs: an accumulator that is not 0 and takes no step"
    assert any(ref.step_of(D, lr) == 0 for D in Ds) and any(D == 0 for D in Ds), "inputs: items with step 0"
    assert clamped, "inputs: a delta beyond 2^40 is clamped"
    if staged:
        assert set().union(*(_stages_of(b, thr) for b in boards)) == {0, 1, 2}, "inputs: the boards lie in all three stages"
    if source != "board":
        lens = np.concatenate([r.len for r in rings])
        assert (np.minimum(lens & 0x7f, H) < H).any() and ((lens & 0x7f) >= H).any(), "inputs: boards with fewer than H valid slots, and full ones"
        assert (rings[-1].len & tref.ENDED).any() and not (rings[-1].len & tref.ENDED).all(), "inputs: episodes that ended at the last push"
        assert not staged or max(spans) > 0, "inputs: a board whose valid slots lie in different stages"


# ------------------------------------------------------------------------------------------------ the device
def dev(torch, a):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda:0")


def device_state(g, torch, rnet, rtc=None):
    """(NTupleNet, NTupleTC or None) on the GPU with the lists, stages, weights and accumulators of a reference network."""
    net = g.NTupleNet(rnet.tuples, frac_bits=rnet.frac_bits, stages=rnet.thr or None, mixed=True)
    net.weights.copy_(torch.as_tensor(mref.flat_of(rnet).astype(np.int32)).reshape(net.weights.shape))
    if rtc is None:
        return net, None
    tc = g.NTupleTC(net)
    err, mag = mref.tc_flat(rtc, rnet)
    tc.err.copy_(torch.as_tensor(err).reshape(tc.err.shape))
    tc.mag.copy_(torch.as_tensor(mag).reshape(tc.mag.shape))
    return net, tc


def tables(net, tc=None):
    """The device's arrays as flat int64, as ntuple_mixed_helpers.want_tables gives the reference's."""
    w = net.weights.cpu().numpy().astype(np.int64).reshape(-1)
    return (w,) if tc is None else (w, tc.err.cpu().numpy().reshape(-1), tc.mag.cpu().numpy().reshape(-1))


def assert_ring_equal(dl, rdl, where=""):
    assert dl.slot == rdl.slot, where
    for name, got, want in (("hist", dl.hist, rdl.hist), ("len", dl.len, rdl.len), ("acc", dl.acc, rdl.acc_i64())):
        assert np.array_equal(got.cpu().numpy(), want), f"{where}: {name}"


def replay_delay(g, torch, run, splits=(ALTERNATE,)):
    """A delay_reference run on the device: ring, accumulators and delta after every push, the tables after every update and
    the ring unchanged by it.  The TD update runs on one network; the TC update on one network (and accumulators) per entry of
    ``splits``, as one call with phases=3 or as two (phases=1, then 2) where the entry says so for the push (None: the flush)."""
    dl = g.NTupleDelay(run.n, depth=run.depth, lam=run.lam / 65536)
    assert dl.lam_q16 == run.lam and dl.slot == run.depth - 1 and not dl.len.any() and not dl.acc.any()
    rnet, rtc = run.state()
    base = want_tables(rnet, rtc if run.tc_form else None)
    td, _ = device_state(g, torch, rnet)
    tcs = [device_state(g, torch, rnet, rtc) for _ in splits] if run.tc_form else []
    out = torch.empty(run.n, dtype=torch.int64, device="cuda")
    for call in run.calls:
        where, p = call.where, call.push
        if p is not None:
            assert dl.push(dev(torch, p.after), dev(torch, p.after_value), dev(torch, p.best_next), dev(torch, p.terminated), out) is out
            assert np.array_equal(out.cpu().numpy(), p.delta), f"{where}: delta"
            assert_ring_equal(dl, call.ring, where)
        td.delay_update(dl, run.lr_shift, flush=bool(call.mode))
        assert_tables_equal(tables(td), call.td.on(base[:1]), names=(f"{where}: td weights",))
        for split, (tcn, tc) in zip(splits, tcs):
            for phases in ((1, 2) if split(call.t) else (3,)):
                tcn.tc_delay_update(dl, run.lr_shift, tc, phases=phases, flush=bool(call.mode))
            assert_tables_equal(tables(tcn, tc), call.tc.on(base), names=tuple(f"{where}: tc {x}" for x in ("weights", "err", "mag")))
        assert_ring_equal(dl, call.ring, where + ": the update wrote to the ring")
    return td, tcs


def run_against_reference(g, torch, n, H, lam, rnet, pushes, seed, lr_shift=10, boards=None, span=1 << 40, tc_form=True):
    """``pushes`` synthetic pushes; each is followed by the TD update on one network and by TC W + A on another (one call with
    phases=3 on even pushes, two calls on odd ones), then the FLUSH: everything against the reference after every call.
    Returns the number of afterstates applied by STEP updates and by the FLUSH, counted in the reference, and its ring."""
    inputs = [(row[0] if boards is None else boards[t],) + tuple(row[1:]) for t, row in enumerate(push_inputs(n, pushes, seed, span=span))]
    run = delay_reference(n, H, lam, lambda: (rnet.copy(), random_tc(rnet, seed + 1) if tc_form else None), inputs, lr_shift, tc_form)
    replay_delay(g, torch, run)
    return run.applied, run.ring
