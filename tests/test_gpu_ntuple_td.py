"""GPU: the fused n-tuple TD step and trainer (g2048_ntuple_td_step, g2048_ntuple_td_train) against the
composition they replace -- td_evaluate(fused=False) and the trainers built on it, on a second engine with the same seed.
Compared bit for bit with torch.equal: the six outputs of every step; after the last step the records as raw bytes, the clock,
episode_stats() in full, the terminal records and their scores, and the records after 20 ordinary steps on both engines, which
shows that the clock and the episode slots were left right; for the trainers also the weights, the TC accumulators and the
trace or delay ring.  The composition itself is tied to the pure-Python reference by the existing n-tuple tests; the fused body
is tied to it on the host by test_ntuple_td_host.py.

Instantiations of ntuple_td_step_kernel<T, Shape> the module runs: NtupleShape, NtupleStagedShape (S = 3) at T = 1..8 and
NtupleMixedShape (S = 3) at T = 2..8 -- 23 of the 24 compiled; the mixed shape at T = 1 cannot be selected (a network of one
list is never mixed)."""
import ctypes as C
import types

import numpy as np
import pytest

import late_game as lg
from ntuple_deep_helpers import family_net, w32_of
from ntuple_play_helpers import ENGINEERED_CLOCK
from ntuple_td_helpers import small_case, start_of, uniform_case

pytestmark = pytest.mark.gpu
SEED = 77
FIELDS = ("action", "after", "after_value", "best_next", "terminated", "delta")


@pytest.fixture(scope="module")
def g(torch_cuda):
    import gym2048_amd
    return gym2048_amd


# ------------------------------------------------------------------------------------------------ networks and engines
def net_of(g, torch, case, fresh=False):
    """The NTupleNet of a case with its weights on the device; ``fresh``: a new one (a trainer changes it), else one per case."""
    if fresh or not hasattr(case, "td_dev"):
        net = g.NTupleNet(case.tuples, frac_bits=case.rnet.frac_bits, stages=case.stages, mixed=True)
        net.weights.copy_(torch.from_numpy(np.ascontiguousarray(case.w32)).reshape(net.weights.shape))
        if fresh:
            return net
        case.td_dev = net
    return case.td_dev


_family_cases = {}


def family_case(family, T):
    """Network T of a family of ntuple_deep_helpers (TUPLES_8x4[:T] or ntuple_mixed_ref.MIX_8[:T]; staged and mixed: three
    stages on the low thresholds; full-range random int32) as a case for net_of."""
    if (family, T) not in _family_cases:
        rnet = family_net(family, T)
        _family_cases[family, T] = types.SimpleNamespace(name=f"{family}-{T}", rnet=rnet, w32=w32_of(rnet).reshape(-1), tuples=tuple(rnet.tuples),
                                                         stages=getattr(rnet, "thr", None))
    return _family_cases[family, T]


def engine(g, n, late, seed=SEED, board_offset=None, **kw):
    """An engine of n boards after reset(), or (``late``) holding ntuple_td_helpers.start_of(n) at ENGINEERED_CLOCK."""
    if board_offset is None:
        board_offset = lg.BASE_OFFSET if late else 0
    eng = g.Batched2048(n, seed=seed, board_offset=board_offset, **kw)
    if late:
        boards, scores = start_of(n)
        eng.set_boards(boards)
        eng.set_scores(scores.astype(np.int32))
        eng.set_clock(ENGINEERED_CLOCK)
    else:
        eng.reset()
    return eng


def pair(g, n, late, **kw):
    return engine(g, n, late, **kw), engine(g, n, late, **kw)


def close(*engines):
    for e in engines:
        e.close()


def state(eng):
    keeps = eng.last_records_enabled
    return types.SimpleNamespace(records=eng.records().clone(), clock=eng.clock, stats=eng.episode_stats(),
                                 last=eng.last_records().clone() if keeps else None, scores=eng.last_scores().clone() if keeps else None)


def assert_engines_equal(a, b, where):
    import torch
    sa, sb = state(a), state(b)
    assert torch.equal(sa.records, sb.records), f"{where}: records differ on boards {torch.nonzero((sa.records != sb.records).any(1))[:8, 0].tolist()}"
    assert sa.clock == sb.clock, f"{where}: clock {sa.clock} vs {sb.clock}"
    assert sa.stats == sb.stats, f"{where}: episode_stats {sa.stats} vs {sb.stats}"
    assert (sa.last is None) == (sb.last is None)
    if sa.last is not None:
        assert torch.equal(sa.last, sb.last), f"{where}: last_records"
        assert torch.equal(sa.scores, sb.scores), f"{where}: last_scores"


def assert_engines_equal_and_stay_equal(a, b, where):
    assert_engines_equal(a, b, where)
    for _ in range(20):
        a.step(None)
        b.step(None)
    assert_engines_equal(a, b, where + ", 20 steps later")


def outputs(eng, work):
    return {"action": work.before.action, "after": work.before.after, "after_value": work.before.after_value, "best_next": work.after.best,
            "terminated": eng.terminated, "delta": work.delta}


def assert_steps_equal(g, fused, composed, net, k, where):
    """k steps either way, the six outputs compared after every step; returns how many (board, step) pairs terminated."""
    import torch
    from gym2048_amd import ntuple
    wf, wc = ntuple.td_work(fused), ntuple.td_work(composed)
    ended = 0
    for j in range(k):
        ntuple.td_evaluate(fused, net, wf, fused=True)
        ntuple.td_evaluate(composed, net, wc, fused=False)
        got, want = outputs(fused, wf), outputs(composed, wc)
        for name in FIELDS:
            assert torch.equal(got[name], want[name]), f"{where}, step {j}: {name} differs on boards " \
                                                        f"{torch.nonzero((got[name] != want[name]).reshape(len(want[name]), -1).any(1))[:8, 0].tolist()}"
        ended += int(want["terminated"].sum())
    return ended


# ------------------------------------------------------------------------------------------------ 1. fused == composition
@pytest.mark.parametrize("late", [True, False], ids=["late-game", "reset"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_fused_equals_composition(g, torch_cuda, n, late):
    net = net_of(g, torch_cuda, small_case())
    a, b = pair(g, n, late)
    ended = assert_steps_equal(g, a, b, net, 40, f"n={n}")
    assert not late or ended >= 1                                   # board 0 of the late-game boards has no legal move
    assert_engines_equal_and_stay_equal(a, b, f"n={n}")
    close(a, b)


@pytest.mark.parametrize("late", [True, False], ids=["late-game", "reset"])
def test_max_tile_is_honoured(g, torch_cuda, late):
    net = net_of(g, torch_cuda, uniform_case())
    a, b = pair(g, 257, late, max_tile=256)
    ended = assert_steps_equal(g, a, b, net, 40, "max_tile=256")
    if late:                                                        # (a reset board does not reach 256 in 40 moves)
        from gym2048_amd import ntuple
        c, plain = engine(g, 257, late), 0
        work = ntuple.td_work(c)
        for _ in range(40):
            ntuple.td_evaluate(c, net, work)
            plain += int(c.terminated.sum())
        assert ended > plain, "inputs: the limit ended episodes that run on without it"
        close(c)
    assert_engines_equal_and_stay_equal(a, b, "max_tile=256")
    close(a, b)


@pytest.mark.parametrize("late", [True, False], ids=["late-game", "reset"])
def test_an_engine_without_terminal_records(g, torch_cuda, late):
    net = net_of(g, torch_cuda, uniform_case())
    a, b = pair(g, 257, late, last_records=False)
    assert not a.last_records_enabled
    ended = assert_steps_equal(g, a, b, net, 40, "no terminal records")
    assert ended >= 1
    assert_engines_equal_and_stay_equal(a, b, "no terminal records")
    close(a, b)


# ------------------------------------------------------------------------------------------------ 2. every instantiation
FAMILY_CASES = [(f, T) for f in ("uniform", "staged") for T in range(1, 9)] + [("mixed", T) for T in range(2, 9)]


@pytest.mark.parametrize("family, T", FAMILY_CASES, ids=[f"{f}-{T}" for f, T in FAMILY_CASES])
def test_every_instantiation(g, torch_cuda, family, T):
    case = family_case(family, T)
    net = net_of(g, torch_cuda, case)
    assert net.n_tuples == T and (net.mixed, net.n_stages) == {"uniform": (False, 1), "staged": (False, 3), "mixed": (True, 3)}[family]
    a, b = pair(g, 65, True)
    ended = assert_steps_equal(g, a, b, net, 8, f"{family} T={T}")
    assert ended >= 1
    assert_engines_equal(a, b, f"{family} T={T}")
    close(a, b)


# ------------------------------------------------------------------------------------------------ 3. the trainers
def assert_states_equal(a, b, where):
    import torch
    assert a.keys() == b.keys()
    for key in a:
        if isinstance(a[key], torch.Tensor):
            assert torch.equal(a[key], b[key]), f"{where}: {key}"
        else:
            assert a[key] == b[key], f"{where}: {key}"


TRAINERS = ["train", "tc_train", "tdl_train", "tcl_train", "delayed_tdl_train", "delayed_tcl_train"]
N_TRAIN, K_TRAIN, LR = 300, 30, 4


def run_trainer(g, torch, name, case, fused, late):
    """One trainer on a fresh engine, network and learner state: (engine, net, tc or None, history or None)."""
    from gym2048_amd import ntuple
    eng, net = engine(g, N_TRAIN, late), net_of(g, torch, case, fresh=True)
    tc = g.NTupleTC(net) if "tc" in name else None
    hist = None
    if "delayed" in name:
        hist = g.NTupleDelay(N_TRAIN, depth=3, lam=0.5)
    elif name.startswith(("tdl", "tcl")):
        hist = g.NTupleTrace(N_TRAIN, depth=3, lam=0.5)
    args = [eng, net] + ([tc] if tc is not None else []) + ([hist] if hist is not None else []) + [K_TRAIN, LR]
    getattr(ntuple, name)(*args, fused=fused)
    return eng, net, tc, hist


def assert_runs_equal(got, want, where):
    assert_states_equal(got[1].state_dict(), want[1].state_dict(), where + ": net")
    if want[2] is not None:
        assert_states_equal(got[2].state_dict(), want[2].state_dict(), where + ": tc")
    if want[3] is not None:
        assert_states_equal(got[3].state_dict(), want[3].state_dict(), where + ": history")
    assert_engines_equal_and_stay_equal(got[0], want[0], where)


@pytest.mark.parametrize("name", TRAINERS)
def test_trainers_fused_equal_composed(g, torch_cuda, name):
    case = small_case()
    got, want = run_trainer(g, torch_cuda, name, case, True, True), run_trainer(g, torch_cuda, name, case, False, True)
    start = net_of(g, torch_cuda, case)
    assert not torch_cuda.equal(want[1].weights, start.weights), "inputs: the run learns something"
    assert want[0].episode_stats()["episodes"] >= 1
    assert_runs_equal(got, want, name)
    close(got[0], want[0])


@pytest.mark.parametrize("name", ["train", "tc_train"])
@pytest.mark.parametrize("family, T", [("staged", 5), ("mixed", 8)])
def test_trainers_on_staged_and_mixed_networks(g, torch_cuda, name, family, T):
    case = family_case(family, T)
    got, want = run_trainer(g, torch_cuda, name, case, True, True), run_trainer(g, torch_cuda, name, case, False, True)
    assert not torch_cuda.equal(want[1].weights, net_of(g, torch_cuda, case).weights)
    assert_runs_equal(got, want, f"{name} {family}")
    close(got[0], want[0])


@pytest.mark.parametrize("with_tc", [False, True], ids=["td", "tc"])
def test_one_train_call_is_k_calls_of_one_step(g, torch_cuda, with_tc):
    from gym2048_amd import ntuple
    case, runs = small_case(), []
    for calls, k in ((1, K_TRAIN), (K_TRAIN, 1)):
        eng, net = engine(g, N_TRAIN, False), net_of(g, torch_cuda, case, fresh=True)
        tc = g.NTupleTC(net) if with_tc else None
        work = ntuple.td_work(eng)
        for _ in range(calls):
            eng.ntuple_td_train(net, work, k, LR, tc)
        runs.append((eng, net, tc, None, work))
    for name, a, b in zip(FIELDS, outputs(runs[0][0], runs[0][4]).values(), outputs(runs[1][0], runs[1][4]).values()):
        assert torch_cuda.equal(a, b), f"work {name} after the last step"
    assert_runs_equal(runs[0], runs[1], "k_steps=30 vs 30 x k_steps=1")
    # k_steps == 0 changes nothing
    eng, net = runs[0][0], runs[0][1]
    before, weights = state(eng), net.weights.clone()
    eng.ntuple_td_train(net, runs[0][4], 0, LR, runs[0][2])
    assert state(eng).clock == before.clock and torch_cuda.equal(eng.records(), before.records) and torch_cuda.equal(net.weights, weights)
    close(runs[0][0], runs[1][0])


# ------------------------------------------------------------------------------------------------ 4. two shards are the whole
def test_two_shards_are_the_whole(g, torch_cuda):
    from gym2048_amd import ntuple
    case = small_case()
    whole, net_w = engine(g, 300, False), net_of(g, torch_cuda, case, fresh=True)
    shards, net_s = [engine(g, 150, False, board_offset=off) for off in (0, 150)], net_of(g, torch_cuda, case, fresh=True)
    works = [ntuple.td_work(e) for e in shards]
    work = ntuple.td_work(whole)
    for _ in range(20):
        ntuple.td_step(whole, net_w, LR, work, fused=True)
        for e, w in zip(shards, works):
            ntuple.td_evaluate(e, net_s, w, fused=True)
        for w in works:
            ntuple.td_update(net_s, w, LR)
    assert torch_cuda.equal(net_s.weights, net_w.weights)
    assert not torch_cuda.equal(net_w.weights, net_of(g, torch_cuda, case).weights)
    assert torch_cuda.equal(torch_cuda.cat([e.records() for e in shards]), whole.records())
    for name in FIELDS:
        parts = torch_cuda.cat([outputs(e, w)[name] for e, w in zip(shards, works)])
        assert torch_cuda.equal(parts, outputs(whole, work)[name]), name
    sw, ss = whole.episode_stats(), [e.episode_stats() for e in shards]
    for key in ("episodes", "illegal_ends", "return_sum"):
        assert sw[key] == ss[0][key] + ss[1][key], key
    close(whole, *shards)


# ------------------------------------------------------------------------------------------------ 5. outputs left NULL
SENTINEL = 0xA5


def sentinel_buffers(torch, n):
    shapes = {"action": ((n,), torch.uint8), "after": ((n, 16), torch.uint8), "after_value": ((n,), torch.int64),
              "best_next": ((n,), torch.int64), "terminated": ((n,), torch.uint8), "delta": ((n,), torch.int64)}
    return {name: torch.full((int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size(),), SENTINEL, dtype=torch.uint8,
                             device="cuda:0").view(dtype).reshape(shape) for name, (shape, dtype) in shapes.items()}


def raw_td_step(g, eng, net, bufs, given):
    from gym2048_amd import _lib
    io = _lib.NTupleTDIO(**{name: bufs[name].data_ptr() for name in given})
    _lib.check(net._fn("td_step")(eng._h, net._ref(eng.device), C.byref(io), eng._stream()))


SUBSETS = [FIELDS[0::2], FIELDS[1::2]] + [tuple(f for f in FIELDS if f != leave) for leave in FIELDS] + [(f,) for f in FIELDS]


@pytest.mark.parametrize("given", SUBSETS, ids=["+".join(s) for s in SUBSETS])
def test_outputs_left_null_are_not_written(g, torch_cuda, given):
    torch = torch_cuda
    net = net_of(g, torch, uniform_case())
    full_eng, eng = pair(g, 65, True)
    full, bufs = sentinel_buffers(torch, 65), sentinel_buffers(torch, 65)
    raw_td_step(g, full_eng, net, full, FIELDS)
    raw_td_step(g, eng, net, bufs, given)
    torch.cuda.synchronize()
    for name in FIELDS:
        if name in given:
            assert torch.equal(bufs[name], full[name]), f"{name}: differs from the call with every output"
        else:
            assert bool((bufs[name].reshape(-1).view(torch.uint8) == SENTINEL).all()), f"{name} was left NULL and its guard was written"
    assert int(full["terminated"].sum()) >= 1 and bool((full["action"] != SENTINEL).all())
    assert_engines_equal(eng, full_eng, "+".join(given))
    close(full_eng, eng)


@pytest.mark.parametrize("n", [65, 257])
def test_all_outputs_null_is_ntuple_play_of_one_step(g, torch_cuda, n):
    net = net_of(g, torch_cuda, uniform_case())
    a, b = pair(g, n, True)
    bufs = sentinel_buffers(torch_cuda, n)
    for _ in range(3):
        raw_td_step(g, a, net, bufs, ())
        b.ntuple_play(net, 1)
    torch_cuda.cuda.synchronize()
    assert all(bool((t.reshape(-1).view(torch_cuda.uint8) == SENTINEL).all()) for t in bufs.values())
    assert a.episode_stats()["episodes"] >= 1
    assert_engines_equal_and_stay_equal(a, b, "all outputs NULL")
    close(a, b)


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_fused_with_a_carousel_raises(g, torch_cuda):
    from gym2048_amd import ntuple
    case = family_case("staged", 2)
    net, eng = net_of(g, torch_cuda, case, fresh=True), engine(g, 64, False)
    carousel = g.Carousel(net, 64, capacity=16)
    tc, trace, delay = g.NTupleTC(net), g.NTupleTrace(64, depth=2), g.NTupleDelay(64, depth=2)
    work = ntuple.td_work(eng)
    before, weights = state(eng), net.weights.clone()
    calls = [(ntuple.td_evaluate, (eng, net, work)), (ntuple.td_step, (eng, net, LR, work)), (ntuple.train, (eng, net, 2, LR)),
             (ntuple.tc_step, (eng, net, tc, LR, work)), (ntuple.tc_train, (eng, net, tc, 2, LR)),
             (ntuple.tdl_evaluate, (eng, net, trace, work)), (ntuple.tdl_step, (eng, net, trace, LR, work)),
             (ntuple.tdl_train, (eng, net, trace, 2, LR)), (ntuple.tcl_step, (eng, net, tc, trace, LR, work)),
             (ntuple.tcl_train, (eng, net, tc, trace, 2, LR)), (ntuple.delayed_evaluate, (eng, net, delay, work)),
             (ntuple.delayed_tdl_step, (eng, net, delay, LR, work)), (ntuple.delayed_tdl_train, (eng, net, delay, 2, LR)),
             (ntuple.delayed_tcl_step, (eng, net, tc, delay, LR, work)), (ntuple.delayed_tcl_train, (eng, net, tc, delay, 2, LR))]
    for fn, args in calls:
        with pytest.raises(ValueError, match="fused=True cannot run a carousel"):
            fn(*args, carousel=carousel, fused=True)
    after = state(eng)
    assert after.clock == before.clock and torch_cuda.equal(after.records, before.records) and torch_cuda.equal(net.weights, weights)
    assert trace.slot == 1 and delay.slot == 1                       # (no push was made: the slot of "the last push" is depth - 1)
    close(eng)


def test_numpy_rng_mode_is_refused(g, torch_cuda):
    from gym2048_amd import ntuple
    net = net_of(g, torch_cuda, uniform_case())
    eng = g.Batched2048(64, seed=SEED, rng="numpy")
    eng.reset()
    work = ntuple.td_work(eng)
    before = state(eng)
    with pytest.raises(g.G2048Error, match="g2048_ntuple_td_step needs the spawn stream: this engine is in numpy-RNG mode"):
        ntuple.td_evaluate(eng, net, work, fused=True)
    with pytest.raises(g.G2048Error, match="g2048_ntuple_td_train needs the spawn stream: this engine is in numpy-RNG mode"):
        ntuple.train(eng, net, 2, LR, fused=True)
    with pytest.raises(g.G2048Error, match="play it with g2048_ntuple_evaluate and g2048_step"):
        ntuple.tc_train(eng, net, g.NTupleTC(net), 2, LR, fused=True)
    after = state(eng)
    assert after.clock == before.clock and torch_cuda.equal(after.records, before.records)
    ntuple.td_evaluate(eng, net, work)                                # the composition remains for that mode
    assert eng.clock == before.clock + 1
    close(eng)
