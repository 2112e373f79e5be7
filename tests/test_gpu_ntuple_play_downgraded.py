"""GPU: downgraded n-tuple play (g2048_ntuple_play_downgraded) -- the fused launch against the composed loop of
its contract on a second engine with the same seed: downgraded_boards -> NTupleNet.evaluate of those plain boards ->
play_step of its action, with the same side outputs.  Compared bit for bit: the records as raw bytes, the clock,
episode_stats() in full, the terminal records, games_left, hist and moves.  One network is also held against the reference
model tests/downgrade_ref.py, from which alone the guard against a vacuous pass is computed.

Instantiations of ntuple_play_downgraded_kernel<T, Shape> the module runs: all 24 -- NtupleShape, NtupleStagedShape (S = 3) and
NtupleMixedShape (S = 3) at T = 1..8.  The mixed shape at T = 1 is reached by describing the one list with a tuple_len longer
than the list (its list then ends early, which is what makes a descriptor mixed); NTupleNet itself never builds that
descriptor.  These tests fail without the feature: ``ntuple_play`` takes no ``downgrade``."""
import types

import numpy as np
import pytest

import downgrade_ref as dref
import late_game as lg
import ntuple_play_ref as pref
import ntuple_staged_ref as sref
from downgrade_helpers import FLOOR_EXP, MIN_EXP, THR_3, net_of, small_case, trace_of

pytestmark = pytest.mark.gpu
SEED = 77
N, K = 130, 120         # two wavefronts and a part; moves from reset


@pytest.fixture(scope="module")
def g(torch_cuda):
    import gym2048_amd
    return gym2048_amd


def rule_of(g, min_exp=MIN_EXP, floor_exp=FLOOR_EXP):
    return g.Downgrade(1 << min_exp, 1 << floor_exp)


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


def side(torch, eng, left=None):
    """(games_left, hist, moves) on the engine's device: the budgets of ``left`` (None: no limit), zeroed counts."""
    d = eng.device
    return (None if left is None else torch.from_numpy(np.ascontiguousarray(left, np.uint32).view(np.int32)).to(d).view(torch.uint32),
            torch.zeros(32, dtype=torch.int64, device=d).view(torch.uint64), torch.zeros(1, dtype=torch.int64, device=d).view(torch.uint64))


def compose(torch, g, eng, net, rule, k, io=(None, None, None)):
    """k rounds of the contract's loop; returns (board-steps with k != 0, board-steps among them whose action differs from the
    plain board's), counted on this trusted path with one host read at the end."""
    from gym2048_amd.ntuple import NTupleEval
    n, d = eng.n_envs, eng.device
    left, hist, moves = io
    low = g.Downgraded(torch.empty((n, 16), dtype=torch.uint8, device=d), torch.empty(n, dtype=torch.uint8, device=d))
    act, plain = torch.empty(n, dtype=torch.uint8, device=d), torch.empty(n, dtype=torch.uint8, device=d)
    counts = torch.zeros(2, dtype=torch.int64, device=d)
    for _ in range(k):
        eng.downgraded_boards(rule, active=left, out=low)
        net.evaluate(low.boards, out=NTupleEval(None, act, None, None, None))
        eng.ntuple_evaluate(net, out=NTupleEval(None, plain, None, None, None))
        on = (low.missing != 0) & (low.missing != 0xff)
        counts[0] += on.sum()
        counts[1] += (on & (act != plain)).sum()
        eng.play_step(act, games_left=left, hist=hist, moves=moves)
    return tuple(counts.tolist())


def state(eng):
    return types.SimpleNamespace(records=eng.records().cpu().numpy().copy(), clock=eng.clock, stats=eng.episode_stats(),
                                 last=eng.last_records().cpu().numpy().copy())


def assert_engines_equal(a, b, where):
    sa, sb = state(a), state(b)
    assert np.array_equal(sa.records, sb.records), f"{where}: records differ on boards {np.nonzero((sa.records != sb.records).any(1))[0][:8]}"
    assert sa.clock == sb.clock, f"{where}: clock {sa.clock} vs {sb.clock}"
    assert sa.stats == sb.stats, f"{where}: episode_stats {sa.stats} vs {sb.stats}"
    assert np.array_equal(sa.last, sb.last), f"{where}: last_records"


def assert_sides_equal(torch, a, b, where):
    for name, x, y in zip(("games_left", "hist", "moves"), a, b):
        assert (x is None) == (y is None) and (x is None or torch.equal(x.view(torch.int32), y.view(torch.int32))), f"{where}: {name}"


def close(*engines):
    for e in engines:
        e.close()


# ------------------------------------------------------------------------------------------------ every instantiation
CASES = [(family, T) for family in ("uniform", "staged", "mixed") for T in range(1, 9)]


@pytest.mark.parametrize("family, T", CASES, ids=[f"{f}-{T}" for f, T in CASES])
def test_fused_is_the_composed_loop(g, torch_cuda, family, T):
    """130 boards, 120 moves from reset, min_exp = 5 and floor_exp = 4, random int32 weights within +-2^12: without a budget, then
    with games_left in {1, 2}, hist and moves."""
    torch = torch_cuda
    case = small_case(family, T)
    net, rule = net_of(g, torch, case), rule_of(g)
    assert net.n_tuples == T and net.n_stages == (1 if family == "uniform" else 3)
    a, b = engine(g, N), engine(g, N)
    a.ntuple_play(net, K, downgrade=rule)
    at_work, changed = compose(torch, g, b, net, rule, K)
    assert at_work >= 100 and changed >= 10, f"{case.name}: the rule was at work on {at_work} board-steps and changed {changed} moves"
    assert_engines_equal(a, b, case.name)
    for _ in range(20):
        a.step(None)
        b.step(None)
    assert_engines_equal(a, b, case.name + ", 20 steps later")
    close(a, b)
    budget = np.random.default_rng(T).integers(1, 3, N).astype(np.uint32)
    a, b = engine(g, N), engine(g, N)
    io_a, io_b = side(torch, a, budget), side(torch, b, budget)
    a.ntuple_play(net, K, games_left=io_a[0], hist=io_a[1], moves=io_a[2], downgrade=rule)
    compose(torch, g, b, net, rule, K, io_b)
    assert_engines_equal(a, b, case.name + ", budgets")
    assert_sides_equal(torch, io_a, io_b, case.name)
    assert int(io_a[1].view(torch.int64).sum()) >= 1 and 0 < int(io_a[2].view(torch.int64)[0]) <= N * K
    close(a, b)


# ------------------------------------------------------------------------------------------------ the reference model
def test_against_the_reference_model_and_the_guard(g, torch_cuda):
    """The counts that show the rule at work come from the Python model alone: at least 100 board-steps with k != 0, and on at
    least 10 of them an action other than the plain board's.  The fused launch then equals the model, with and without budgets."""
    torch = torch_cuda
    case = small_case("uniform", 1)             # (one tuple: the pure-Python model plays these 15 600 moves in a few seconds)
    tr = trace_of(case, N, K, SEED)
    on = tr.missing != 0
    assert on.sum() >= 100 and (tr.action[on] != tr.plain_action[on]).sum() >= 10
    net, rule = net_of(g, torch, case), rule_of(g)
    for budget in (None, np.random.default_rng(2).integers(1, 3, N).astype(np.uint32)):
        want = pref.limited(tr, budget)
        assert want.episodes.sum() >= 1 and (budget is None or (want.games_left == 0).any())
        eng = engine(g, N)
        left, hist, moves = side(torch, eng, budget)
        stats0 = eng.episode_stats()
        eng.ntuple_play(net, K, games_left=left, hist=hist, moves=moves, downgrade=rule)
        st = eng.episode_stats()
        assert np.array_equal(eng.records().cpu().numpy(), want.records) and eng.clock == want.clock
        assert st["episodes"] - stats0["episodes"] == int(want.episodes.sum()) and st["return_sum"] - stats0["return_sum"] == want.return_sum
        had = want.episodes > 0
        assert np.array_equal(eng.last_records().cpu().numpy()[had], want.last_records[had])
        if budget is not None:
            assert np.array_equal(left.view(torch.int32).cpu().numpy().view(np.uint32), want.games_left)
        assert np.array_equal(hist.view(torch.int64).cpu().numpy(), want.hist.astype(np.int64)) and int(moves.view(torch.int64)[0]) == want.moves
        close(eng)


# ------------------------------------------------------------------------------------------------ identity, large tiles, stages
def test_min_exp_31_is_ntuple_play(g, torch_cuda):
    torch = torch_cuda
    for family, T in (("uniform", 5), ("staged", 3), ("mixed", 4)):
        net = net_of(g, torch, small_case(family, T))
        a, b = engine(g, N), engine(g, N)
        a.ntuple_play(net, K, downgrade=g.Downgrade(1 << 31, 16))
        b.ntuple_play(net, K)
        assert_engines_equal(a, b, f"{family}-{T}")
        close(a, b)


def test_boards_with_32768_65536_and_131072(g, torch_cuda):
    """The engineered late-game boards (exponents 12..17 at every fill level, pairs of 2^16 and 2^17 that merge) under the default
    rule -- at work from the 32768 tile on -- at a non-zero board_offset and a clock above 2^32: fused against composed."""
    torch = torch_cuda
    fam = lg.high_family(lg.SEED, n=512)
    exps = fam.boards.max(axis=1)
    assert all((exps == e).sum() >= 16 for e in (15, 16, 17))
    rule = g.Downgrade()
    assert (dref.downgrade(fam.boards, 15, 4)[1] != 0).sum() >= 100
    start = (fam.boards, fam.scores, (1 << 32) + 1000)
    for family, T in (("uniform", 4), ("staged", 5), ("mixed", 8)):
        net = net_of(g, torch, small_case(family, T))
        a = engine(g, 512, seed=lg.SEED, start=start, board_offset=lg.BASE_OFFSET)
        b = engine(g, 512, seed=lg.SEED, start=start, board_offset=lg.BASE_OFFSET)
        a.ntuple_play(net, 12, downgrade=rule)
        at_work, _ = compose(torch, g, b, net, rule, 12)
        assert at_work >= 100
        assert_engines_equal(a, b, f"high tiles, {family}-{T}")
        close(a, b)


def test_a_translated_board_in_an_earlier_stage(g, torch_cuda):
    """Boards that hold a 64 and no 32: the board is in stage 2 of (16 | 64), its translation -- the 64 halved -- in stage 1.  One
    move: where the model's action on the translated board differs from the plain player's, the fused launch makes the
    model's move and ntuple_play makes the other."""
    torch = torch_cuda
    case = small_case("staged", 4)
    rng = np.random.default_rng(31)
    boards = np.where(rng.random((256, 16)) < 0.35, 0, rng.integers(1, 4, (256, 16))).astype(np.uint8)   # 2, 4 and 8: no 16 that could block k = 5
    boards[:, 5] = 6
    low, k = dref.downgrade(boards, MIN_EXP, FLOOR_EXP)
    assert (k == 5).all() and (sref.stage_batch(boards, THR_3) == 2).all() and (sref.stage_batch(low, THR_3) == 1).all()
    start = lambda: pref.start_of(256, SEED, boards=boards, clock=500)                       # noqa: E731
    tr = dref.unlimited(start(), 1, case.rnet, MIN_EXP, FLOOR_EXP)
    plain = pref.unlimited(start(), 1, case.rnet)
    differ = (tr.action[0] != plain.action[0]) & (tr.after[0] != plain.after[0]).any(axis=1)   # another move, and another board for it
    assert differ.sum() >= 10
    net = net_of(g, torch, case)
    a = engine(g, 256, start=(boards, np.zeros(256, np.int32), 500))
    b = engine(g, 256, start=(boards, np.zeros(256, np.int32), 500))
    a.ntuple_play(net, 1, downgrade=rule_of(g))
    b.ntuple_play(net, 1)
    assert np.array_equal(a.records().cpu().numpy(), pref.limited(tr).records)
    assert np.array_equal(b.records().cpu().numpy(), pref.limited(plain).records)
    assert (a.records().cpu().numpy()[differ] != b.records().cpu().numpy()[differ]).any(axis=1).all()
    close(a, b)


def test_refusals_and_the_empty_call(g, torch_cuda):
    torch = torch_cuda
    net, rule = net_of(g, torch, small_case("uniform", 5)), rule_of(g)
    numpy_eng = g.Batched2048(64, seed=SEED, rng="numpy")
    numpy_eng.reset()
    with pytest.raises(g.G2048Error, match="numpy-RNG"):
        numpy_eng.ntuple_play(net, 4, downgrade=rule)
    eng = engine(g, 64)
    before = state(eng)
    eng.ntuple_play(net, 0, downgrade=rule)                         # k_steps = 0: nothing changes
    with pytest.raises(ValueError, match="Downgrade"):
        eng.ntuple_play(net, 4, downgrade=(5, 4))
    after = state(eng)
    assert np.array_equal(before.records, after.records) and before.clock == after.clock and before.stats == after.stats
    close(eng, numpy_eng)
