"""GPU: n-tuple play (g2048_ntuple_play) -- the fused launch against the composition it replaces,
ntuple_evaluate -> step on a second engine with the same seed, and against the reference model tests/ntuple_play_ref.py on
the smaller cases.  Compared bit for bit: the records as raw bytes, the clock, episode_stats() in full, the terminal
records, and the records after 20 ordinary steps on both engines, which shows that the clock and the episode slots were
left right.  Budgets (games_left) have no composition: their expectation is derived, by the reference model's ``limited``,
from the trace of the composition on the trusted per-move path, or from the reference's own trace.

Instantiations of ntuple_play_kernel<T, Shape> the module runs: NtupleShape at T = 1..8 (test_every_tuple_count),
NtupleStagedShape at T = 1..8 and NtupleMixedShape at T = 2..8, both with S = 3 (test_every_staged_and_mixed_instantiation; before
it the staged shape ran at T = 5 alone and the mixed one at T = 8 alone, with S = 1) -- 23 of the 24 compiled.  NOT reached: the
mixed shape at T = 1; NTupleNet takes tuple_len from the longest list, so a network of one list is never mixed and the Python
layer cannot select it.  Measured on the MI355X's host: the module takes 7.1 s on its own; the 15 tests of
test_every_staged_and_mixed_instantiation take 1 s together, the slowest 0.2 s."""
import ctypes as C
import types

import numpy as np
import pytest

import late_game as lg
import ntuple_play_ref as pref
import ntuple_staged_ref as sref
from ntuple_deep_helpers import family_net, w32_of
from ntuple_play_helpers import (ENGINEERED_CLOCK, budgets, engineered, engineered_trace, mixed_case, staged_case, trace_of,
                                 uniform_case)

pytestmark = pytest.mark.gpu
SEED = 77
K_BLOCK = 256           # kBlock of g2048_kernels.hip (asserted against the source below)
K_GAIN_FOLD = 1024      # kGainFold


@pytest.fixture(scope="module")
def g(torch_cuda):
    import gym2048_amd
    return gym2048_amd


def test_the_constants_are_the_source_s():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gym-2048_amd", "csrc", "g2048_kernels.hip")).read()
    assert int(re.search(r"constexpr int kBlock = (\d+);", src).group(1)) == K_BLOCK
    assert int(re.search(r"constexpr uint32_t kGainFold = (\d+);", src).group(1)) == K_GAIN_FOLD


def net_of(g, torch, case):
    """The NTupleNet of a case with its weights on the device (cached on the case: one upload per network)."""
    if not hasattr(case, "dev"):
        net = g.NTupleNet(case.tuples, frac_bits=case.rnet.frac_bits, stages=case.stages, mixed=True)
        net.weights.copy_(torch.from_numpy(case.w32).reshape(net.weights.shape))
        case.dev = net
    return case.dev


def engine(g, n, seed=SEED, start=None, **kw):
    eng = g.Batched2048(n, seed=seed, **kw)
    if start is None:
        eng.reset()
    else:
        boards, scores, clock = start
        eng.set_boards(boards)
        eng.set_scores(scores)
        eng.set_clock(clock)
    return eng


def compose(eng, net, k):
    """k rounds of ntuple_evaluate -> step(action, auto_reset): what the fused launch must equal."""
    import torch
    from gym2048_amd.ntuple import NTupleEval
    out = NTupleEval(None, torch.empty(eng.n_envs, dtype=torch.uint8, device=eng.device), None, None, None)
    for _ in range(k):
        eng.step(eng.ntuple_evaluate(net, out=out).action, want_info=False)


def u32(t):
    """A uint32 device tensor as a numpy array."""
    import torch
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def i64(t):
    """A uint64 device tensor as a numpy int64 array."""
    import torch
    return t.view(torch.int64).cpu().numpy()


def state(eng):
    return types.SimpleNamespace(records=eng.records().cpu().numpy().copy(), clock=eng.clock, stats=eng.episode_stats(),
                                 last=eng.last_records().cpu().numpy().copy() if eng.last_records_enabled else None)


def assert_engines_equal(a, b, where):
    sa, sb = state(a), state(b)
    assert np.array_equal(sa.records, sb.records), f"{where}: records differ on boards {np.nonzero((sa.records != sb.records).any(1))[0][:8]}"
    assert sa.clock == sb.clock, f"{where}: clock {sa.clock} vs {sb.clock}"
    assert sa.stats == sb.stats, f"{where}: episode_stats {sa.stats} vs {sb.stats}"
    assert (sa.last is None) == (sb.last is None) and (sa.last is None or np.array_equal(sa.last, sb.last)), f"{where}: last_records"


def assert_fused_is_composition(fused, composed, net, k, where):
    """Play k steps either way, compare, then 20 ordinary steps on both and compare again."""
    fused.ntuple_play(net, k)
    compose(composed, net, k)
    assert_engines_equal(fused, composed, where)
    for _ in range(20):
        fused.step(None)
        composed.step(None)
    assert_engines_equal(fused, composed, where + ", 20 steps later")


def pair(g, n, **kw):
    return engine(g, n, **kw), engine(g, n, **kw)


def close(*engines):
    for e in engines:
        e.close()


# ------------------------------------------------------------------------------------------------ geometry and step counts
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("n", [1, 63, 64, 65, K_BLOCK + 1])
def test_fused_equals_composition(g, torch_cuda, n, k):
    net = net_of(g, torch_cuda, uniform_case())
    a, b = pair(g, n)
    assert_fused_is_composition(a, b, net, k, f"n={n} k={k}")
    close(a, b)


def test_one_step_past_the_gain_fold(g, torch_cuda):
    net = net_of(g, torch_cuda, uniform_case())
    a, b = pair(g, 65)
    assert_fused_is_composition(a, b, net, K_GAIN_FOLD + 1, "k=1025")
    assert a.episode_stats()["episodes"] > 65                        # games ended on both sides of the fold
    close(a, b)


@pytest.mark.parametrize("T", range(1, 9))
def test_every_tuple_count(g, torch_cuda, T):
    net = net_of(g, torch_cuda, uniform_case(T))
    a, b = pair(g, 65)
    assert_fused_is_composition(a, b, net, 300, f"T={T}")
    assert a.episode_stats()["episodes"] >= 65
    close(a, b)


@pytest.mark.parametrize("name", ["staged", "mixed", "zero"])
def test_every_shape(g, torch_cuda, name):
    case = {"staged": staged_case, "mixed": mixed_case, "zero": lambda: uniform_case(zero=True)}[name]()
    net = net_of(g, torch_cuda, case)
    assert (net.n_stages, net.mixed) == {"staged": (3, False), "mixed": (1, True), "zero": (1, False)}[name]
    a, b = pair(g, 65)
    assert_fused_is_composition(a, b, net, 300, name)
    assert a.episode_stats()["episodes"] >= (1 if name == "zero" else 65)
    close(a, b)


FAMILY_CASES = [("staged", T) for T in range(1, 9)] + [("mixed", T) for T in range(2, 9)]
_family_cases = {}


def family_case(family, T):
    """Network T of a family of ntuple_deep_helpers (TUPLES_8x4[:T] or ntuple_mixed_ref.MIX_8[:T], three stages on the low
    thresholds, full-range random int32) as a case for net_of."""
    if (family, T) not in _family_cases:
        rnet = family_net(family, T)
        _family_cases[family, T] = types.SimpleNamespace(name=f"{family}-{T}", rnet=rnet, w32=w32_of(rnet).reshape(-1), tuples=tuple(rnet.tuples),
                                                         stages=rnet.thr)
    return _family_cases[family, T]


@pytest.mark.parametrize("family, T", FAMILY_CASES, ids=[f"{f}-{T}" for f, T in FAMILY_CASES])
def test_every_staged_and_mixed_instantiation(g, torch_cuda, family, T):
    """The staged and the mixed player at every tuple count, S = 3, 65 boards: the fused launch against the composition.  The
    evaluate kernel the composition leans on is tied to the pure-Python reference for exactly these networks by
    test_gpu_ntuple_search_matrix.py::test_evaluate_and_values_of_staged_and_mixed_networks.  k is the smallest number of steps
    after which 65 episodes have ended, found on the composed (trusted) path, whose records -- every eighth step's -- are shown
    by ntuple_staged_ref.stage_batch to lie in at least two stages."""
    case = family_case(family, T)
    net = net_of(g, torch_cuda, case)
    assert net.n_tuples == T and (net.mixed, net.n_stages) == {"staged": (False, 3), "mixed": (True, 3)}[family]
    scout, k, seen = engine(g, 65), 0, []
    while scout.episode_stats()["episodes"] < 65:
        assert k < 1000, "no 65 episodes in 1000 steps"
        if k % 8 == 0:
            seen.append(scout.records().cpu().numpy().copy())
        compose(scout, net, 1)
        k += 1
    seen.append(scout.records().cpu().numpy().copy())
    close(scout)
    assert len(set(sref.stage_batch(np.concatenate(seen), case.stages).tolist())) >= 2, "inputs: the boards lie in at least two stages"
    a, b = pair(g, 65)
    assert_fused_is_composition(a, b, net, k, f"{family} T={T} k={k}")
    assert a.episode_stats()["episodes"] >= 65
    close(a, b)


# ------------------------------------------------------------------------------------------------ the reference model
def assert_matches_reference(eng, want, left, hist, moves, stats0, where):
    """The engine after a fused run against ntuple_play_ref.limited's result."""
    st = eng.episode_stats()
    assert np.array_equal(eng.records().cpu().numpy(), want.records), f"{where}: records"
    assert eng.clock == want.clock, where
    assert st["episodes"] - stats0["episodes"] == int(want.episodes.sum()), where
    assert st["return_sum"] - stats0["return_sum"] == want.return_sum, where
    had = want.episodes > 0
    assert np.array_equal(eng.last_records().cpu().numpy()[had], want.last_records[had]), f"{where}: last_records"
    if left is not None:
        assert np.array_equal(u32(left), want.games_left), f"{where}: games_left"
    assert np.array_equal(i64(hist), want.hist.astype(np.int64)), f"{where}: hist"
    assert int(i64(moves)[0]) == want.moves, f"{where}: moves"


def side(torch, eng, left=None):
    """(games_left, hist, moves) on the engine's device: the budgets of ``left`` (None: no limit), zeroed counts."""
    dev = eng.device
    return (None if left is None else torch.from_numpy(np.ascontiguousarray(left, np.uint32).view(np.int32)).to(dev).view(torch.uint32),
            torch.zeros(32, dtype=torch.int64, device=dev).view(torch.uint64), torch.zeros(1, dtype=torch.int64, device=dev).view(torch.uint64))


@pytest.mark.parametrize("name, k", [("17x4", 130), ("staged", 160)])
@pytest.mark.parametrize("limited", [False, True], ids=["unlimited", "budgets"])
def test_against_the_reference_model(g, torch_cuda, name, k, limited):
    torch = torch_cuda
    case = uniform_case() if name == "17x4" else staged_case()
    tr = trace_of(case, 64, k, SEED)
    budget = budgets(64, 5) if limited else None
    want = pref.limited(tr, budget)
    hit = pref.reaches(tr, want)
    assert hit.two_episodes and hit.directions == {0, 1, 2, 3} and (not limited or (hit.ran_out and hit.never_moved))
    eng = engine(g, 64)
    left, hist, moves = side(torch, eng, budget)
    stats0 = eng.episode_stats()
    eng.ntuple_play(net_of(g, torch, case), k, games_left=left, hist=hist, moves=moves)
    assert_matches_reference(eng, want, left, hist, moves, stats0, name)
    close(eng)


def test_engineered_boards(g, torch_cuda):
    """One empty cell, full and terminal boards (action 0, illegal, the episode ends on it) and the score-deficit carry, at a
    non-zero board_offset and a clock above 2^32: against the reference, with and without budgets, and the composition."""
    torch, case, k = torch_cuda, uniform_case(), 12
    net = net_of(g, torch, case)
    tr = engineered_trace(case, k)
    boards, scores, dead, _ = engineered()
    start = (boards, scores, ENGINEERED_CLOCK)
    for budget in (None, np.full(96, 2, np.uint32), budgets(96, 6)):
        want = pref.limited(tr, budget)
        eng = engine(g, 96, seed=lg.SEED, start=start, board_offset=lg.BASE_OFFSET)
        left, hist, moves = side(torch, eng, budget)
        stats0 = eng.episode_stats()
        eng.ntuple_play(net, k, games_left=left, hist=hist, moves=moves)
        assert_matches_reference(eng, want, left, hist, moves, stats0, "engineered")
        illegal_ends = eng.episode_stats()["illegal_ends"] - stats0["illegal_ends"]
        assert illegal_ends == int((tr.illegal & want.played).sum()) and (budget is not None or illegal_ends >= 12)
        close(eng)
    a = engine(g, 96, seed=lg.SEED, start=start, board_offset=lg.BASE_OFFSET)
    b = engine(g, 96, seed=lg.SEED, start=start, board_offset=lg.BASE_OFFSET)
    assert_fused_is_composition(a, b, net, k, "engineered")
    close(a, b)


# ------------------------------------------------------------------------------------------------ other engine settings
def test_max_tile_ends_episodes(g, torch_cuda):
    net = net_of(g, torch_cuda, uniform_case())
    a, b = pair(g, 65, max_tile=64)
    assert_fused_is_composition(a, b, net, 120, "max_tile=64")
    st = a.episode_stats()
    assert st["episodes"] > 65 and st["max_exp"] <= 6                # every game ends on reaching 64 (or earlier)
    close(a, b)


def test_an_engine_without_terminal_records(g, torch_cuda):
    net = net_of(g, torch_cuda, uniform_case())
    a, b = pair(g, 65, last_records=False)
    assert not a.last_records_enabled
    assert_fused_is_composition(a, b, net, 300, "last_records=False")
    assert a.episode_stats()["episodes"] >= 65
    close(a, b)


def test_two_halves_are_the_whole(g, torch_cuda):
    torch = torch_cuda
    net = net_of(g, torch, uniform_case())
    whole, lo, hi = engine(g, 130, board_offset=1000), engine(g, 65, board_offset=1000), engine(g, 65, board_offset=1065)
    budget = budgets(130, 9)
    sides = [side(torch, e, b) for e, b in ((whole, budget), (lo, budget[:65]), (hi, budget[65:]))]
    for e, (left, hist, moves) in zip((whole, lo, hi), sides):
        e.ntuple_play(net, 300, games_left=left, hist=hist, moves=moves)
    rec = [e.records().cpu().numpy() for e in (whole, lo, hi)]
    assert np.array_equal(rec[0], np.concatenate(rec[1:]))
    assert np.array_equal(u32(sides[0][0]), np.concatenate([u32(sides[1][0]), u32(sides[2][0])]))
    assert np.array_equal(i64(sides[0][1]), i64(sides[1][1]) + i64(sides[2][1])) and i64(sides[0][1]).sum() > 65
    assert i64(sides[0][2]) == i64(sides[1][2]) + i64(sides[2][2])
    st = [e.episode_stats() for e in (whole, lo, hi)]
    for key in ("episodes", "illegal_ends", "return_sum"):
        assert st[0][key] == st[1][key] + st[2][key], key
    assert np.array_equal(whole.last_records().cpu().numpy(), np.concatenate([lo.last_records().cpu().numpy(), hi.last_records().cpu().numpy()]))
    # the same boards without a budget, on an engine with an offset, are the composition
    a, b = pair(g, 65, board_offset=1065)
    assert_fused_is_composition(a, b, net, 100, "board_offset")
    close(whole, lo, hi, a, b)


# ------------------------------------------------------------------------------------------------ budgets
def composed_trace(torch, eng, net, k):
    """The unlimited trace (as ntuple_play_ref.unlimited's) of k rounds of evaluate -> step on the per-move path."""
    n = eng.n_envs
    rec = lambda: eng.records().cpu().numpy().copy()
    tr = types.SimpleNamespace(n=n, k=k, t0=eng.clock, start=rec(), action=np.zeros((k, n), np.uint8), terminated=np.zeros((k, n), bool),
                               illegal=np.zeros((k, n), bool), gain=np.zeros((k, n), np.int64), after=np.zeros((k, n, 16), np.uint8),
                               terminal=np.zeros((k, n, 16), np.uint8), terminal_score=np.zeros((k, n), np.int64))
    for j in range(k):
        act = eng.ntuple_evaluate(net).action
        eng.step(act)
        tr.action[j], tr.terminated[j], tr.illegal[j] = act.cpu().numpy(), eng.terminated.cpu().numpy() != 0, eng.illegal.cpu().numpy() != 0
        tr.gain[j] = np.where(tr.illegal[j], 0, eng.reward.cpu().numpy()).astype(np.int64)
        tr.after[j] = rec()
        done = tr.terminated[j]
        tr.terminal[j][done] = eng.last_records().cpu().numpy()[done]
        tr.terminal_score[j][done] = eng.get_last_scores()[done]
    return tr


def head(tr, k):
    """The first k steps of a trace."""
    out = types.SimpleNamespace(**vars(tr))
    out.k = k
    for name in ("action", "terminated", "illegal", "gain", "after", "terminal", "terminal_score"):
        setattr(out, name, getattr(tr, name)[:k])
    return out


def test_budgets_over_two_launches(g, torch_cuda):
    torch, n, k1, k2 = torch_cuda, 257, 120, 180
    net = net_of(g, torch, uniform_case())
    ref_eng = engine(g, n)
    tr = composed_trace(torch, ref_eng, net, k1 + k2)
    budget = budgets(n, 11)
    assert all((budget == v).sum() >= 16 for v in (0, 1, 2, pref.NO_LIMIT))
    mid, want = pref.limited(head(tr, k1), budget), pref.limited(tr, budget)
    hit = pref.reaches(tr, want)
    assert hit.ran_out and hit.never_moved and hit.two_episodes
    assert ((mid.games_left == 0) & (budget > 0)).any() and ((want.games_left == 0) & (mid.games_left > 0)).any()   # budgets run out in both launches

    eng = engine(g, n)
    left, hist, moves = side(torch, eng, budget)
    total = lambda t: int(u32(t).astype(np.int64).sum())
    stats0, left0 = eng.episode_stats(), total(left)
    eng.ntuple_play(net, k1, games_left=left, hist=hist, moves=moves)
    stats1, left1, rec1 = eng.episode_stats(), total(left), eng.records().cpu().numpy().copy()
    assert np.array_equal(u32(left), mid.games_left) and np.array_equal(i64(hist), mid.hist.astype(np.int64))
    assert i64(hist).sum() == left0 - left1 == stats1["episodes"] - stats0["episodes"] > 0 and int(i64(moves)[0]) == mid.moves
    resting = u32(left) == 0
    eng.ntuple_play(net, k2, games_left=left, hist=hist, moves=moves)           # accumulates into the same hist and moves
    stats2 = eng.episode_stats()
    assert i64(hist).sum() == left0 - total(left) == stats2["episodes"] - stats0["episodes"] > stats1["episodes"] - stats0["episodes"]
    assert resting.sum() > (budget == 0).sum() and np.array_equal(eng.records().cpu().numpy()[resting], rec1[resting])
    assert_matches_reference(eng, want, left, hist, moves, stats0, "two launches")
    assert eng.clock == ref_eng.clock == tr.t0 + k1 + k2               # the clock moved by k1 + k2 whatever the budgets were
    close(eng, ref_eng)


# ------------------------------------------------------------------------------------------------ play_games
def test_play_games_reports_every_board_s_first_game(g, torch_cuda):
    torch, n = torch_cuda, 256
    case = uniform_case(T=1)
    score, top, length = pref.first_games(n, SEED, case.rnet, cap=2000)
    assert (score >= 0).all() and length.max() > 128 and length.min() < 64
    net = net_of(g, torch, case)
    eng = engine(g, n)
    eng.step(None)
    eng.seed(SEED)                                                   # the clock back to 0: the games are a function of seed and clock
    report = g.play_games(eng, net, games=1, chunk=64)
    assert report.games == n and report.unfinished == 0
    assert np.array_equal(report.scores.cpu().numpy(), score)
    assert report.mean_score == int(score.sum()) / n
    hist = np.bincount(top, minlength=32)
    assert report.hist == hist.tolist() and report.reach == pref.reach_of(hist) and report.moves == int(length.sum())
    assert set(report.reach) == set(pref.REACH_TILES)
    # too few steps: the games that are over are reported, the others are owed
    eng.seed(SEED)
    short = g.play_games(eng, net, games=1, chunk=32, max_steps=64)
    over = length <= 64
    assert 0 < over.sum() < n and short.games == int(over.sum()) and short.unfinished == n - short.games > 0
    assert short.mean_score == int(score[over].sum()) / short.games and short.hist == np.bincount(top[over], minlength=32).tolist()
    assert short.moves == int(np.minimum(length, 64).sum())
    # two games per board: no per-game scores, exactly 2n games
    two = g.play_games(eng, net, games=2, chunk=256)
    assert two.games == 2 * n and two.unfinished == 0 and two.scores is None and sum(two.hist) == 2 * n
    close(eng)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_and_the_empty_call(g, torch_cuda):
    torch = torch_cuda
    from gym2048_amd import _lib
    net = net_of(g, torch, uniform_case())
    numpy_eng = g.Batched2048(64, seed=SEED, rng="numpy")
    numpy_eng.reset()
    with pytest.raises(g.G2048Error, match="numpy-RNG"):
        numpy_eng.ntuple_play(net, 4)
    eng = engine(g, 64)
    before = state(eng)
    eng.ntuple_play(net, 0)                                          # k_steps = 0: nothing changes
    left, hist, moves = side(torch, eng, np.ones(64, np.uint32))
    eng.ntuple_play(net, 0, games_left=left, hist=hist, moves=moves)
    after = state(eng)
    assert np.array_equal(before.records, after.records) and before.clock == after.clock and before.stats == after.stats
    assert int(left.view(torch.int32).sum()) == 64 and not hist.view(torch.int64).any() and not moves.view(torch.int64).any()
    lib, ref_ = _lib.load(), net._ref(eng.device)
    for field, offset in (("hist", 4), ("moves", 4), ("games_left", 2)):
        io = _lib.NTuplePlayIO(left.data_ptr(), hist.data_ptr(), moves.data_ptr())
        setattr(io, field, getattr(io, field) + offset)
        assert lib.g2048_ntuple_play(eng._h, ref_, 4, C.byref(io), None) == -1 and b"misaligned" in lib.g2048_last_error()
    after = state(eng)
    assert np.array_equal(before.records, after.records) and before.clock == after.clock
    close(eng, numpy_eng)
