"""GPU: the n-tuple move log and backward learning (g2048_ntuple_play_log, g2048_ntuple_log_delta, g2048_ntuple_log_sweep,
g2048_ntuple_log_train), bit for bit with torch.equal:

* play_log against the composition it replaces -- ntuple_evaluate -> step on a twin engine with the same seed -- slot by slot
  over two consecutive calls (the second shows the carry), the engines compared as test_gpu_ntuple_td.py compares them
  (records, clock, episode_stats(), terminal records, 20 ordinary steps afterwards), one case with max_tile, sentinel bytes
  behind slot M untouched; for n <= 257 also against the pure-Python reference (tests/ntuple_log_ref.py);
* log_delta against NTupleNet.values on the slot views plus integer arithmetic, for every m, under the log's own flags and
  under flags overwritten with all 256 byte values;
* log_sweep and backward_train against the hand-made sequence of existing calls and against the Python reference: the
  weights, the TC accumulators, delta after the last position, the log; TD, TC and mean=; two rounds of the C trainer against
  two rounds of the Python one;
* two shards, each with its own log, against one engine of the whole;
* NULL members, bad depths and the numpy-RNG engine through the Python layer.

n = 1, 65, 257 and 1 000; M = 1, 2 and 6.  Every test first asserts from the reference alone (never from the code under
test) that its case holds what it names.  The instantiations of both kernels are in test_gpu_ntuple_log_matrix.py."""
import ctypes as C

import numpy as np
import pytest

import ntuple_log_ref as lref
import ntuple_mean_ref as meanref
import ntuple_play_ref as pref
import ntuple_tc_ref as tcref
from ntuple_play_helpers import ENGINEERED_CLOCK
from ntuple_log_helpers import (SENTINEL, all_flag_bytes, assert_device_logs_equal, assert_engines_equal, assert_engines_equal_and_stay_equal,
                                assert_log_case, close, composed_play_log, engine, family_case, guarded_log, load_log, net_of,
                                one_stage_case, state, values_delta)
from ntuple_td_helpers import CASES, small_case, uniform_case

pytestmark = pytest.mark.gpu
ROUNDS = 2


@pytest.fixture(scope="module")
def g(torch_cuda):
    import gym2048_amd
    return gym2048_amd


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


# ------------------------------------------------------------------------------------------------ 1. play_log == composition
def run_play_log_pair(g, torch, case, n, M, where, **kw):
    """Two play_log calls on one engine against two composed rounds on its twin: every slot after each call, the guards, the
    engines.  Returns the logs (device) after each call."""
    net = net_of(g, torch, case)
    weights = net.weights.clone()
    a, b = engine(g, n, **kw), engine(g, n, **kw)
    log, guards = guarded_log(g, torch, n, M)
    want = g.NTupleLog(n, depth=M)
    seen = []
    for r in range(ROUNDS):
        a.ntuple_play_log(net, log)
        composed_play_log(b, net, want)
        assert_device_logs_equal(log, want, f"{where}, call {r}")
        seen.append(log.state_dict())
    assert not bool(seen[0]["flag"][0].any()), "first call: slot 0 stays empty"
    for name in ("after", "gain", "flag"):
        assert torch.equal(seen[1][name][0], seen[0][name][M]), f"{where}: the second call carries {name} of slot M into slot 0"
    # (slot-major: the bytes past board n of slot m < M are board 0 of slot m + 1, compared above; past board n of slot M are these)
    for name, guard in guards.items():
        assert bool((guard == SENTINEL).all()), f"{where}: bytes behind slot M of {name} were written"
    assert torch.equal(net.weights, weights), "the weights are only read"
    assert_engines_equal_and_stay_equal(a, b, where)
    close(a, b)
    return seen


@pytest.mark.parametrize("M", [1, 2, 6])
@pytest.mark.parametrize("n", [1, 65, 257, 1000])
def test_play_log_equals_composition(g, torch_cuda, n, M):
    case = small_case()
    if n <= 257:
        _, logs = lref.frozen_rounds(case, n, M, ROUNDS)
        assert_log_case(logs, n, M)
    seen = run_play_log_pair(g, torch_cuda, case, n, M, f"n={n} M={M}")
    if n <= 257:                                                       # ... and the Python reference
        for r in range(ROUNDS):
            for name in ("flag", "gain", "after"):
                assert torch_cuda.equal(seen[r][name], dev(torch_cuda, getattr(logs[r], name))), f"n={n} M={M} call {r}: {name} vs reference"
    else:
        flags = torch_cuda.cat([s["flag"][1:].reshape(-1) for s in seen])
        assert set(flags.unique().tolist()) == {0, 1, 3}


@pytest.mark.parametrize("name", ["17x4", "staged", "mixed"])
def test_play_log_on_every_kind_of_network(g, torch_cuda, name):
    case = CASES[name]()
    _, logs = lref.frozen_rounds(case, 65, 6, ROUNDS)
    assert_log_case(logs, 65, 6)
    seen = run_play_log_pair(g, torch_cuda, case, 65, 6, name)
    for r in range(ROUNDS):
        for field in ("flag", "gain", "after"):
            assert torch_cuda.equal(seen[r][field], dev(torch_cuda, getattr(logs[r], field))), f"{name} call {r}: {field} vs reference"


def test_max_tile_is_honoured(g, torch_cuda):
    case = uniform_case()
    want, logs = lref.frozen_rounds(case, 257, 6, ROUNDS, max_exp=8)
    plain, _ = lref.frozen_rounds(case, 257, 6, ROUNDS)
    assert want.episodes > plain.episodes, "inputs: the limit ends episodes that run on without it"
    seen = run_play_log_pair(g, torch_cuda, case, 257, 6, "max_tile=256", max_tile=256)
    for r in range(ROUNDS):
        assert torch_cuda.equal(seen[r]["flag"], dev(torch_cuda, logs[r].flag)), f"call {r}: flag vs reference"


def test_an_engine_without_terminal_records(g, torch_cuda):
    run_play_log_pair(g, torch_cuda, uniform_case(), 257, 2, "no terminal records", last_records=False)


def test_play_log_is_ntuple_play(g, torch_cuda):
    """The contract in one sentence: the engine ends in the bits of ntuple_play(net, M)."""
    net = net_of(g, torch_cuda, uniform_case())
    a, b = engine(g, 1000), engine(g, 1000)
    log = g.NTupleLog(1000, depth=6)
    for _ in range(3):
        a.ntuple_play_log(net, log)
        b.ntuple_play(net, 6)
    assert a.episode_stats()["episodes"] >= 1
    assert_engines_equal_and_stay_equal(a, b, "play_log vs ntuple_play")
    close(a, b)


# ------------------------------------------------------------------------------------------------ 2. log_delta
@pytest.mark.parametrize("n", [1, 65, 257, 1000])
def test_log_delta_is_values_and_integer_arithmetic(g, torch_cuda, n):
    torch = torch_cuda
    case, M = uniform_case(), 6 if n > 1 else 3
    net = net_of(g, torch, case)
    eng, log = engine(g, n), g.NTupleLog(n, depth=M)
    for _ in range(ROUNDS):
        eng.ntuple_play_log(net, log)
    if n <= 257:
        _, logs = lref.frozen_rounds(case, n, M, ROUNDS)
        assert_log_case(logs, n, M)
        assert_device_logs_equal(log, logs[1], f"n={n}")
    before = log.state_dict()
    room = torch.full((n + 64,), 0x5a5a5a5a, dtype=torch.int64, device="cuda:0")   # delta [n] and a guard behind board n
    out, guard = room[:n], room[n:]
    # the log's own flags, then flags that hold every byte value
    wild = dev(torch, all_flag_bytes(M, n))
    assert n == 1 or set(wild.unique().tolist()) == set(range(256))
    for flags, label in ((log.flag.clone(), "own flags"), (wild, "all 256 flag bytes")):
        log.flag.copy_(flags)
        nonzero = 0
        for m in range(M):
            want = values_delta(net, log, m, flags)
            got = net.log_delta(log, m)
            assert torch.equal(got, want), f"n={n} {label} slot {m}: boards {torch.nonzero(got != want)[:8, 0].tolist()}"
            assert net.log_delta(log, m, out=out) is out and torch.equal(out, want)
            if n <= 257 and label == "own flags":
                assert torch.equal(got, dev(torch, lref.log_delta(case.rnet, logs[1], m))), f"n={n} slot {m} vs reference"
            nonzero += int((want != 0).sum())
        assert n == 1 or nonzero >= n
    assert bool((guard == 0x5a5a5a5a).all()), "log_delta wrote past delta[n]"
    log.flag.copy_(before["flag"])
    for name in ("after", "gain", "flag"):
        assert torch.equal(getattr(log, name), before[name]), f"log_delta wrote {name}"
    close(eng)


# ------------------------------------------------------------------------------------------------ 3. sweep and trainer
LR = {"small": 2, "17x4": 8, "17x4-S1": 8}


def reference_sweep(case, n, M, kind):
    """(the reference log of the second round -- its slot 0 is live, so M = 2 updates two slots --, lr_shift, (net, tc, mean,
    delta) after one reference sweep of it); the guards of the issue first."""
    logs = lref.frozen_rounds(case, n, M, ROUNDS)[1][1:]
    lr = LR[{"17x4-small": "small", "5x4": "17x4"}.get(case.name, case.name)]
    results = {}
    for key in ("td", "tc", "mean", "up"):
        if key == "mean" and kind != "mean":
            continue
        if key == "tc" and kind == "mean":
            continue
        net = case.rnet.copy()
        tc = tcref.TC(net) if key == "tc" else None
        mean = meanref.Mean(net) if key == "mean" else None
        delta = lref.sweep(net, logs[0], lr, tc=tc, mean=mean, order=range(M) if key == "up" else None)
        results[key] = (net, tc, mean, delta)
    start, td = case.rnet.weights, results["td"][0].weights
    flat = lambda w: np.asarray(w).reshape(-1, np.asarray(w).shape[-1])   # noqa: E731  (every table of every stage)
    assert all(not np.array_equal(a, b) for a, b in zip(flat(td), flat(start))), "every table of every stage changes"
    if "tc" in results:
        assert not np.array_equal(results["tc"][0].weights, td), "the TC result differs from the TD result"
    assert M == 1 or not np.array_equal(results["up"][0].weights, td), "ascending m gives other weights: the order is under test"
    return logs[0], lr, results[kind]


def hand_made_sweep(net, log, lr, tc=None, mean=None):
    """The 2M (3M) existing calls by hand; returns delta after the last position."""
    delta = None
    for m in range(log.depth - 1, -1, -1):
        delta = net.log_delta(log, m)
        if tc is not None:
            net.tc_update(log.slot(m), delta, lr, tc)
        elif mean is not None:
            net.mean_update(log.slot(m), delta, lr, mean)
        else:
            net.update(log.slot(m), delta, lr)
    return delta


def assert_learners_equal(torch, got, want, where):
    """(net, tc or None) pairs, device against device or against the reference's arrays."""
    as_dev = lambda x, like: x if isinstance(x, torch.Tensor) else dev(torch, np.asarray(x).astype(np.int64)).to(like.dtype).reshape(like.shape)   # noqa: E731
    assert torch.equal(got[0].weights, as_dev(want[0].weights, got[0].weights)), f"{where}: weights"
    if got[1] is not None:
        assert torch.equal(got[1].err, as_dev(want[1].err, got[1].err)), f"{where}: tc err"
        mag = want[1].mag if isinstance(want[1].mag, torch.Tensor) else want[1].mag_i64()
        assert torch.equal(got[1].mag, as_dev(mag, got[1].mag)), f"{where}: tc mag"


@pytest.mark.parametrize("kind", ["td", "tc", "mean"])
@pytest.mark.parametrize("name, n, M", [("small", 65, 6), ("17x4", 65, 2), ("17x4", 257, 6)])
def test_log_sweep_against_the_hand_made_calls_and_the_reference(g, torch_cuda, name, n, M, kind):
    from gym2048_amd import ntuple
    torch = torch_cuda
    case = one_stage_case() if kind == "mean" else CASES[name]()       # (the batch-mean reference is written for a StagedNet)
    rlog, lr, (rnet, rtc, rmean, rdelta) = reference_sweep(case, n, M, kind)
    runs = []
    for by_hand in (False, True):
        net = net_of(g, torch, case)
        tc = g.NTupleTC(net) if kind == "tc" else None
        mean = g.NTupleMean(net) if kind == "mean" else None
        log = load_log(torch, g.NTupleLog(n, depth=M), rlog)
        delta = hand_made_sweep(net, log, lr, tc, mean) if by_hand else ntuple.log_sweep(net, log, lr, tc=tc, mean=mean)
        assert_device_logs_equal(log, rlog, "the sweep only reads the log")
        runs.append((net, tc, delta))
    where = f"{kind} {name} n={n} M={M}"
    assert_learners_equal(torch, runs[0], runs[1], where + ": sweep vs by hand")
    assert torch.equal(runs[0][2], runs[1][2]), where + ": delta after the last position"
    assert_learners_equal(torch, runs[0], (rnet, rtc), where + ": sweep vs reference")
    assert torch.equal(runs[0][2], dev(torch, rdelta)), where + ": delta vs reference"
    if kind == "mean":
        assert rmean.is_zero() and not bool(mean.sum.any()) and not bool(mean.count.any())


@pytest.mark.parametrize("kind", ["td", "tc", "mean"])
@pytest.mark.parametrize("name, n, M", [("small", 65, 2), ("17x4", 65, 6)])
def test_backward_train_against_the_python_trainer(g, torch_cuda, name, n, M, kind):
    """Two rounds of the C trainer (mean=: the Python loop over the same launches) against two rounds of the reference's."""
    from gym2048_amd import ntuple
    torch = torch_cuda
    case = one_stage_case() if kind == "mean" else CASES[name]()
    lr = LR[{"17x4-small": "small", "5x4": "17x4"}.get(case.name, case.name)]
    # the reference, and from it alone: the second round plays under other weights than the first left, and learns
    rnet, rlog, o = case.rnet.copy(), lref.Log(n, M), lref.oracle_of(n)
    rtc = tcref.TC(rnet) if kind == "tc" else None
    rmean = meanref.Mean(rnet) if kind == "mean" else None
    lref.train(o, rnet, rlog, 1, lr, rtc, rmean)
    after_one = np.array(rnet.weights, copy=True)
    rdelta = lref.train(o, rnet, rlog, 1, lr, rtc, rmean)
    assert not np.array_equal(after_one, case.rnet.weights) and not np.array_equal(rnet.weights, after_one)
    assert (rlog.flag[0] != 0).any() and {1, 3} <= {int(f) for f in np.unique(rlog.flag)}   # a carried slot 0; entries that ended
    net, eng, log = net_of(g, torch, case), engine(g, n), g.NTupleLog(n, depth=M)
    tc = g.NTupleTC(net) if kind == "tc" else None
    mean = g.NTupleMean(net) if kind == "mean" else None
    assert ntuple.backward_train(eng, net, log, ROUNDS, lr, tc=tc, mean=mean) is net
    where = f"{kind} {name} n={n} M={M}"
    assert_learners_equal(torch, (net, tc), (rnet, rtc), where)
    assert_device_logs_equal(log, rlog, where)
    assert torch.equal(eng.records(), dev(torch, pref.records_of(o.boards, o.score))), where + ": records"
    assert eng.clock == ENGINEERED_CLOCK + ROUNDS * M
    if kind != "mean":                                                  # delta after the last position: the C trainer's work buffer
        delta = torch.zeros(n, dtype=torch.int64, device="cuda:0")
        net2, eng2, log2 = net_of(g, torch, case), engine(g, n), g.NTupleLog(n, depth=M)
        tc2 = g.NTupleTC(net2) if kind == "tc" else None
        eng2.ntuple_log_train(net2, log2, ROUNDS, lr, delta, tc2)
        assert torch.equal(delta, dev(torch, rdelta)), where + ": delta"
        assert_learners_equal(torch, (net2, tc2), (net, tc), where + ": ntuple_log_train vs backward_train")
        close(eng2)
    close(eng)


@pytest.mark.parametrize("kind", ["td", "tc", "mean"])
@pytest.mark.parametrize("family, T", [("uniform", 5), ("staged", 5), ("mixed", 8)])
def test_backward_train_is_the_hand_made_loop(g, torch_cuda, family, T, kind):
    """1 000 boards, M = 6, three rounds, full-range weights: one trainer call against play_log and the 2M (3M) existing calls
    per round by hand, and one call of three rounds against three calls of one."""
    from gym2048_amd import ntuple
    torch = torch_cuda
    case, n, M, lr, rounds = family_case(family, T), 1000, 6, 8, 3
    runs = []
    for mode in ("one call", "by hand", "three calls"):
        net, eng, log = net_of(g, torch, case), engine(g, n), g.NTupleLog(n, depth=M)
        tc = g.NTupleTC(net) if kind == "tc" else None
        mean = g.NTupleMean(net) if kind == "mean" else None
        if mode == "one call":
            ntuple.backward_train(eng, net, log, rounds, lr, tc=tc, mean=mean)
        elif mode == "three calls":
            for _ in range(rounds):
                ntuple.backward_train(eng, net, log, 1, lr, tc=tc, mean=mean)
        else:
            for _ in range(rounds):
                eng.ntuple_play_log(net, log)
                hand_made_sweep(net, log, lr, tc, mean)
        runs.append((net, tc, eng, log))
    assert not torch.equal(runs[1][0].weights, net_of(g, torch, case).weights), "inputs: the run learns something"
    assert runs[1][2].episode_stats()["episodes"] >= 1
    for other, label in ((runs[0], "one call"), (runs[2], "three calls")):
        assert_learners_equal(torch, other[:2], runs[1][:2], f"{family} {kind}: {label} vs by hand")
        assert_device_logs_equal(other[3], runs[1][3], f"{family} {kind}: {label}")
        assert_engines_equal(other[2], runs[1][2], f"{family} {kind}: {label}")
    assert_engines_equal_and_stay_equal(runs[0][2], runs[1][2], f"{family} {kind}")
    close(*[r[2] for r in runs])


def test_zero_rounds_change_nothing(g, torch_cuda):
    from gym2048_amd import ntuple
    torch = torch_cuda
    net, eng, log = net_of(g, torch, small_case()), engine(g, 65), g.NTupleLog(65, depth=2)
    ntuple.backward_train(eng, net, log, 1, 2)
    before, weights, logged = state(eng), net.weights.clone(), log.state_dict()
    ntuple.backward_train(eng, net, log, 0, 2)
    ntuple.backward_train(eng, net, log, 0, 2, tc=g.NTupleTC(net))
    ntuple.backward_train(eng, net, log, 0, 2, mean=g.NTupleMean(net))
    after = state(eng)
    assert after.clock == before.clock and torch.equal(after.records, before.records) and torch.equal(net.weights, weights)
    assert all(torch.equal(getattr(log, k), logged[k]) for k in ("after", "gain", "flag"))
    close(eng)


# ------------------------------------------------------------------------------------------------ 4. two shards are the whole
@pytest.mark.parametrize("kind", ["td", "tc"])
def test_two_shards_are_the_whole(g, torch_cuda, kind):
    """Two engines over the two halves, each with its own log, one network: play_log everywhere; then, per m, log_delta on every
    shard, followed by the update on every shard (TC: W everywhere, then A everywhere)."""
    from gym2048_amd import ntuple
    torch = torch_cuda
    case, n, half, M, lr = uniform_case(), 1000, 500, 6, 8
    net_w, whole, log_w = net_of(g, torch, case), engine(g, n), g.NTupleLog(n, depth=M)
    tc_w = g.NTupleTC(net_w) if kind == "tc" else None
    net_s = net_of(g, torch, case)
    tc_s = g.NTupleTC(net_s) if kind == "tc" else None
    shards = [engine(g, half, first=first) for first in (0, half)]
    logs = [g.NTupleLog(half, depth=M) for _ in shards]
    deltas = [torch.empty(half, dtype=torch.int64, device="cuda:0") for _ in shards]
    for _ in range(ROUNDS):
        ntuple.backward_train(whole, net_w, log_w, 1, lr, tc=tc_w)
        for e, log in zip(shards, logs):
            e.ntuple_play_log(net_s, log)
        for m in range(M - 1, -1, -1):
            for log, d in zip(logs, deltas):
                net_s.log_delta(log, m, out=d)
            if kind == "td":
                for log, d in zip(logs, deltas):
                    net_s.update(log.slot(m), d, lr)
            else:
                for phase in (ntuple.TC_WEIGHTS, ntuple.TC_ACCUM):
                    for log, d in zip(logs, deltas):
                        net_s.tc_update(log.slot(m), d, lr, tc_s, phases=phase)
    assert not torch.equal(net_w.weights, net_of(g, torch, case).weights)
    assert_learners_equal(torch, (net_s, tc_s), (net_w, tc_w), f"shards {kind}")
    for name in ("after", "gain", "flag"):
        assert torch.equal(torch.cat([getattr(log, name) for log in logs], dim=1), getattr(log_w, name)), name
    assert torch.equal(torch.cat([e.records() for e in shards]), whole.records())
    sw, ss = whole.episode_stats(), [e.episode_stats() for e in shards]
    assert sw["episodes"] >= 1
    for key in ("episodes", "illegal_ends", "return_sum"):
        assert sw[key] == ss[0][key] + ss[1][key], key
    close(whole, *shards)


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_null_members_and_bad_depths_raise(g, torch_cuda):
    from gym2048_amd import _lib, ntuple
    torch = torch_cuda
    net, eng, log = net_of(g, torch, small_case()), engine(g, 65), g.NTupleLog(65, depth=2)
    delta = torch.zeros(65, dtype=torch.int64, device="cuda:0")
    before, weights = state(eng), net.weights.clone()
    for depth in (0, 1025, -1, 1.5):
        with pytest.raises(ValueError, match="depth"):
            g.NTupleLog(65, depth=depth)
    good = (log.depth, log.after.data_ptr(), log.gain.data_ptr(), log.flag.data_ptr())
    bad = [("log after is NULL", (2, None, good[2], good[3])), ("log gain is NULL", (2, good[1], None, good[3])),
           ("log flag is NULL", (2, good[1], good[2], None)), ("depth=0", (0,) + good[1:]), ("depth=1025", (1025,) + good[1:]),
           ("log after needs 16 bytes", (2, good[1] + 8, good[2], good[3])), ("log gain needs 8 bytes", (2, good[1], good[2] + 4, good[3]))]
    for message, fields in bad:
        log._c = _lib.NTupleLogC(*fields)
        for call in (lambda: eng.ntuple_play_log(net, log), lambda: net.log_delta(log, 0), lambda: ntuple.log_sweep(net, log, 2),
                     lambda: ntuple.backward_train(eng, net, log, 1, 2), lambda: ntuple.backward_train(eng, net, log, 1, 2, tc=g.NTupleTC(net))):
            with pytest.raises(g.G2048Error, match=message):
                call()
    log._c = _lib.NTupleLogC(*good)
    with pytest.raises(g.G2048Error, match="m=2"):                       # (past the Python layer's own check)
        _lib.check(net._fn("log_delta")(65, net._ref(eng.device), C.byref(log._c), 2, delta.data_ptr(), eng._stream()))
    after = state(eng)
    assert after.clock == before.clock and torch.equal(after.records, before.records) and torch.equal(net.weights, weights)
    assert not bool(log.flag.any())
    eng.ntuple_play_log(net, log)                                        # the log and the engine are still good
    assert eng.clock == before.clock + 2 and bool(log.flag.any())
    close(eng)


def test_numpy_rng_mode_is_refused(g, torch_cuda):
    from gym2048_amd import ntuple
    import late_game as lg
    net = net_of(g, torch_cuda, uniform_case())
    eng = g.Batched2048(64, seed=lg.SEED, rng="numpy")
    eng.reset()
    log = g.NTupleLog(64, depth=2)
    before = state(eng)
    with pytest.raises(g.G2048Error, match="g2048_ntuple_play_log needs the spawn stream: this engine is in numpy-RNG mode"):
        eng.ntuple_play_log(net, log)
    with pytest.raises(g.G2048Error, match="g2048_ntuple_log_train needs the spawn stream: this engine is in numpy-RNG mode"):
        ntuple.backward_train(eng, net, log, 2, 4)
    with pytest.raises(g.G2048Error, match="play it with g2048_ntuple_evaluate and g2048_step"):
        ntuple.backward_train(eng, net, log, 2, 4, tc=g.NTupleTC(net))
    with pytest.raises(g.G2048Error, match="numpy-RNG mode"):
        ntuple.backward_train(eng, net, log, 2, 4, mean=g.NTupleMean(net))
    after = state(eng)
    assert after.clock == before.clock and torch_cuda.equal(after.records, before.records) and not bool(log.flag.any())
    close(eng)
