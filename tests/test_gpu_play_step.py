"""GPU: the budgeted play step, the masked search and the game reports built on them (g2048_play_step,
g2048_ntuple_search_active, play_games(depth=, player=)).

Three witnesses of the step.  Without side outputs it is ``step`` on a second engine with the same seed; with actions from
``ntuple_evaluate`` and budgets it is ``ntuple_play`` on a second engine; and with a fixed action table it is the CPU
reference of play_step_helpers (``OracleBatch.step`` traced, then ``ntuple_play_ref.limited``).  Compared bit for bit: the
records as raw bytes, the clock, episode_stats() in full, the terminal records, the side outputs, and the state after 20
ordinary steps on both engines.  The masked search is compared with the unmasked call of the same boards; the reports with
one derived, by ``limited``, from a trace of the per-move composition on a second engine."""
import ctypes as C
import types

import numpy as np
import pytest

import late_game as lg
import ntuple_play_ref as pref
import play_step_helpers as psh
from ntuple_play_helpers import ENGINEERED_CLOCK, budgets, engineered, mixed_case, staged_case, uniform_case
from ntuple_search_helpers import SEARCH_GROUP

pytestmark = pytest.mark.gpu
SEED = psh.SEED
ILLEGAL = -(1 << 63)
SEARCH_MAX_LANES = 1 << 24      # kSearchMaxLanes (g2048_kernels.hip)


@pytest.fixture(scope="module")
def g(torch_cuda):
    import gym2048_amd
    return gym2048_amd


def net_of(g, torch, case):
    """The NTupleNet of an ntuple_play_helpers case with its weights on the device."""
    key = "dev_play_step"
    if not hasattr(case, key):
        net = g.NTupleNet(case.tuples, frac_bits=case.rnet.frac_bits, stages=case.stages, mixed=True)
        net.weights.copy_(torch.from_numpy(case.w32).reshape(net.weights.shape))
        setattr(case, key, net)
    return getattr(case, key)


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


def close(*engines):
    for e in engines:
        e.close()


def u32(t):
    import torch
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def i64(t):
    import torch
    return t.view(torch.int64).cpu().numpy()


def dev_u32(torch, eng, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(eng.device).view(torch.uint32)


def side(torch, eng, left=None, hist0=None, moves0=0):
    """(games_left, hist, moves) on the engine's device: the budgets of ``left`` (None: no limit), the counts at their start."""
    hist = torch.from_numpy(np.zeros(32, np.int64) if hist0 is None else np.asarray(hist0, np.int64)).to(eng.device).view(torch.uint64)
    moves = torch.full((1,), moves0, dtype=torch.int64, device=eng.device).view(torch.uint64)
    return None if left is None else dev_u32(torch, eng, left), hist, moves


def state(eng):
    return types.SimpleNamespace(records=eng.records().cpu().numpy().copy(), clock=eng.clock, stats=eng.episode_stats(),
                                 last=eng.last_records().cpu().numpy().copy() if eng.last_records_enabled else None)


def assert_engines_equal(a, b, where):
    sa, sb = state(a), state(b)
    assert np.array_equal(sa.records, sb.records), f"{where}: records differ on boards {np.nonzero((sa.records != sb.records).any(1))[0][:8]}"
    assert sa.clock == sb.clock, f"{where}: clock {sa.clock} vs {sb.clock}"
    assert sa.stats == sb.stats, f"{where}: episode_stats {sa.stats} vs {sb.stats}"
    assert (sa.last is None) == (sb.last is None) and (sa.last is None or np.array_equal(sa.last, sb.last)), f"{where}: last_records"


def assert_equal_now_and_later(a, b, where):
    assert_engines_equal(a, b, where)
    for _ in range(20):
        a.step(None)
        b.step(None)
    assert_engines_equal(a, b, where + ", 20 steps later")


# ------------------------------------------------------------------------------------------------ io == NULL: the step
@pytest.mark.parametrize("dtype", ["uint8", "int32", "int64", None])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_without_side_outputs_it_is_step(g, torch_cuda, n, dtype):
    """k = 1 and k = 64 (compared after the first step and after the last); actions outside 0..3 play their low two bits."""
    torch = torch_cuda
    table = psh.random_table(64, n, 21).astype(np.int64)
    table[5::7, ::3] += 4                                            # 4..7: the low two bits are played
    if dtype not in (None, "uint8"):
        table[3::11, 1::5] -= 8                                      # negative
    acts = None if dtype is None else torch.from_numpy(table).to("cuda", getattr(torch, dtype))
    a, b = engine(g, n), engine(g, n)
    for j in range(64):
        a.play_step(None if acts is None else acts[j])
        b.step(None if acts is None else acts[j], want_info=False)
        if j == 0:
            assert_engines_equal(a, b, f"n={n} {dtype} k=1")
    assert a.episode_stats()["episodes"] > 0
    assert_equal_now_and_later(a, b, f"n={n} {dtype} k=64")
    close(a, b)


def test_an_engine_without_terminal_records_and_a_list_of_actions(g, torch_cuda):
    a, b = engine(g, 65, last_records=False), engine(g, 65, last_records=False)
    table = psh.random_table(40, 65, 22)
    for j in range(40):
        a.play_step(table[j].tolist())                               # (converted as step converts: int64)
        b.step(table[j].tolist(), want_info=False)
    assert_equal_now_and_later(a, b, "last_records=False")
    close(a, b)


# ------------------------------------------------------------------------------------------------ the second witness
@pytest.mark.parametrize("name", ["uniform", "staged", "mixed"])
def test_with_evaluate_s_actions_and_budgets_it_is_ntuple_play(g, torch_cuda, name):
    torch, n, k = torch_cuda, 65, 160
    net = net_of(g, torch, {"uniform": uniform_case, "staged": staged_case, "mixed": mixed_case}[name]())
    a, b = engine(g, n), engine(g, n)
    budget = budgets(n, 5)
    sa, sb = side(torch, a, budget), side(torch, b, budget)
    out = g.NTupleEval(None, torch.empty(n, dtype=torch.uint8, device=a.device), None, None, None)
    for _ in range(k):
        a.play_step(a.ntuple_evaluate(net, out=out).action, games_left=sa[0], hist=sa[1], moves=sa[2])
    b.ntuple_play(net, k, games_left=sb[0], hist=sb[1], moves=sb[2])
    assert np.array_equal(u32(sa[0]), u32(sb[0])) and np.array_equal(i64(sa[1]), i64(sb[1])) and np.array_equal(i64(sa[2]), i64(sb[2]))
    left = u32(sa[0])
    assert i64(sa[1]).sum() > n // 2 and ((left == 0) & (budget > 0)).any() and (left[budget == pref.NO_LIMIT] < pref.NO_LIMIT).any()   # budgets ran out
    assert_equal_now_and_later(a, b, name)
    close(a, b)


# ------------------------------------------------------------------------------------------------ the CPU reference
def assert_matches_reference(eng, want, left, hist, moves, stats0, where, hist0=None, moves0=0):
    st = eng.episode_stats()
    assert np.array_equal(eng.records().cpu().numpy(), want.records), f"{where}: records"
    assert eng.clock == want.clock, where
    assert st["episodes"] - stats0["episodes"] == int(want.episodes.sum()), where
    assert st["illegal_ends"] - stats0["illegal_ends"] == int(want.illegal_ends), where
    assert st["return_sum"] - stats0["return_sum"] == want.return_sum, where
    had = want.episodes > 0
    assert np.array_equal(eng.last_records().cpu().numpy()[had], want.last_records[had]), f"{where}: last_records"
    if left is not None:
        assert np.array_equal(u32(left), want.games_left), f"{where}: games_left"
    assert np.array_equal(i64(hist), want.hist.astype(np.int64) + (0 if hist0 is None else hist0)), f"{where}: hist"
    assert int(i64(moves)[0]) == want.moves + moves0, f"{where}: moves"


def limited(tr, budget):
    want = pref.limited(tr, budget)
    want.illegal_ends = (tr.illegal & want.terminated).sum()
    return want


def play_table(torch, eng, actions, left, hist, moves):
    acts = torch.from_numpy(actions).to(eng.device)
    for j in range(len(actions)):
        eng.play_step(acts[j], games_left=left, hist=hist, moves=moves)


@pytest.mark.parametrize("n", [65, 257])
def test_the_random_table_against_the_reference(g, torch_cuda, n):
    torch = torch_cuda
    actions, tr = psh.table_trace(n)
    for budget in (budgets(n, 5), None):
        want = limited(tr, budget)
        psh.assert_reaches(tr, want, budget is not None)
        eng = engine(g, n)
        left, hist, moves = side(torch, eng, budget)
        stats0 = eng.episode_stats()
        play_table(torch, eng, actions, left, hist, moves)
        assert_matches_reference(eng, want, left, hist, moves, stats0, f"n={n}")
        close(eng)


def test_engineered_boards_against_the_reference(g, torch_cuda):
    """Dead boards, one hole and the deficit carry, at a clock above 2^32 and a non-zero board_offset."""
    torch = torch_cuda
    actions, tr = psh.engineered_table_trace()
    boards, scores, _, _ = engineered()
    for budget in (None, np.full(96, 2, np.uint32), budgets(96, 6)):
        want = limited(tr, budget)
        eng = engine(g, 96, seed=lg.SEED, start=(boards, scores, ENGINEERED_CLOCK), board_offset=lg.BASE_OFFSET)
        left, hist, moves = side(torch, eng, budget)
        stats0 = eng.episode_stats()
        play_table(torch, eng, actions, left, hist, moves)
        assert_matches_reference(eng, want, left, hist, moves, stats0, "engineered")
        assert budget is not None or want.illegal_ends >= 12
        close(eng)


def test_max_tile_board_offset_and_prefilled_counts(g, torch_cuda):
    torch, n = torch_cuda, 65
    actions, tr = psh.table_trace(n, board_offset=1000, max_exp=4)
    budget = budgets(n, 7)
    want, free = limited(tr, budget), limited(tr, None)
    # max_tile = 16 ends games that an unlimited board would have gone on with: more episodes than without it
    assert free.episodes.sum() > limited(psh.table_trace(n, board_offset=1000)[1], None).episodes.sum()
    assert (tr.terminal[tr.terminated] & 0x1f).max() == 4
    hist0, moves0 = np.arange(32, dtype=np.int64) * 1000 + (1 << 40), (1 << 33) + 5
    eng = engine(g, n, board_offset=1000, max_tile=16)
    left, hist, moves = side(torch, eng, budget, hist0, moves0)
    stats0 = eng.episode_stats()
    play_table(torch, eng, actions, left, hist, moves)
    assert_matches_reference(eng, want, left, hist, moves, stats0, "max_tile", hist0, moves0)        # accumulated, not overwritten
    close(eng)


def test_all_budgets_zero_moves_only_the_clock(g, torch_cuda):
    torch, n = torch_cuda, 65
    eng = engine(g, n)
    for _ in range(3):
        eng.step(None)
    before = state(eng)
    left, hist, moves = side(torch, eng, np.zeros(n, np.uint32))
    bad = torch.full((n,), 200, dtype=torch.uint8, device=eng.device)
    for acts in (None, bad, torch.zeros(n, dtype=torch.int64, device=eng.device)):
        eng.play_step(acts, games_left=left, hist=hist, moves=moves)
    after = state(eng)
    assert np.array_equal(before.records, after.records) and np.array_equal(before.last, after.last) and before.stats == after.stats
    assert after.clock == before.clock + 3
    assert not u32(left).any() and not i64(hist).any() and not i64(moves).any()
    ref = engine(g, n)                                               # the spawn stream moved on by three transactions
    for _ in range(3):
        ref.step(None)
    ref.set_clock(ref.clock + 3)
    assert_equal_now_and_later(eng, ref, "three steps that nobody played")
    close(eng, ref)


def test_two_shards_are_the_whole(g, torch_cuda):
    torch = torch_cuda
    actions, tr = psh.table_trace(130, board_offset=1000)
    budget = budgets(130, 9)
    want = limited(tr, budget)
    whole, lo, hi = engine(g, 130, board_offset=1000), engine(g, 65, board_offset=1000), engine(g, 65, board_offset=1065)
    parts = ((whole, slice(0, 130)), (lo, slice(0, 65)), (hi, slice(65, 130)))
    sides = [side(torch, e, budget[s]) for e, s in parts]
    stats0 = whole.episode_stats()
    for (e, s), (left, hist, moves) in zip(parts, sides):
        play_table(torch, e, np.ascontiguousarray(actions[:, s]), left, hist, moves)
    assert_matches_reference(whole, want, *sides[0], stats0, "whole")
    assert np.array_equal(whole.records().cpu().numpy(), np.concatenate([lo.records().cpu().numpy(), hi.records().cpu().numpy()]))
    assert np.array_equal(u32(sides[0][0]), np.concatenate([u32(sides[1][0]), u32(sides[2][0])]))
    assert np.array_equal(i64(sides[0][1]), i64(sides[1][1]) + i64(sides[2][1])) and i64(sides[0][1]).sum() > 65
    assert i64(sides[0][2]) == i64(sides[1][2]) + i64(sides[2][2])
    st = [e.episode_stats() for e in (whole, lo, hi)]
    for key in ("episodes", "illegal_ends", "return_sum"):
        assert st[0][key] == st[1][key] + st[2][key], key
    close(whole, lo, hi)


# ------------------------------------------------------------------------------------------------ engine settings
def test_strict_actions_report_a_playing_board_only(g, torch_cuda):
    torch, n = torch_cuda, 65
    eng = engine(g, n, strict_actions=True)
    budget = np.full(n, pref.NO_LIMIT, np.uint32)
    budget[40] = 0                                                   # board 40 rests, board 41 plays
    left, hist, moves = side(torch, eng, budget)
    acts = torch.from_numpy(psh.random_table(1, n, 31)[0]).to(eng.device)
    acts[40] = 4
    eng.play_step(acts, games_left=left, hist=hist, moves=moves)     # the 4 is on a resting board: not looked at
    torch.cuda.synchronize()
    eng.get_boards()                                                 # no report
    acts[41] = 4
    clock = eng.clock + 1
    eng.play_step(acts, games_left=left, hist=hist, moves=moves)
    torch.cuda.synchronize()
    with pytest.raises(g.G2048Error, match=r"strict actions.*board 41, low byte 0x04"):
        eng.play_step(acts, games_left=left, hist=hist, moves=moves)
    assert eng.clock == clock                                        # the refused call did nothing
    eng.get_boards()                                                 # reported once; the engine goes on
    # the same for a step made with step(): the two share the report word
    eng.step(acts.to(torch.int32))
    torch.cuda.synchronize()
    with pytest.raises(g.G2048Error, match=r"strict actions.*board 4[01]"):
        eng.get_boards()
    close(eng)


def test_two_chain_engine_gives_the_same_bits(g, torch_cuda):
    torch, n = torch_cuda, 257
    actions, tr = psh.table_trace(n)
    budget = budgets(n, 5)
    want = limited(tr, budget)
    one, two = engine(g, n), engine(g, n, chains=2)
    assert two.chains == 2
    sides = [side(torch, e, budget) for e in (one, two)]
    stats0 = two.episode_stats()
    for e, s in zip((one, two), sides):
        play_table(torch, e, actions, *s)
    assert_matches_reference(two, want, *sides[1], stats0, "chains=2")
    assert all(np.array_equal(i64(x), i64(y)) if x.dtype == torch.uint64 else np.array_equal(u32(x), u32(y)) for x, y in zip(*sides))
    assert_equal_now_and_later(one, two, "chains=2")
    close(one, two)


def test_refusals_that_need_an_engine(g, torch_cuda):
    torch = torch_cuda
    from gym2048_amd import _lib
    lib = _lib.load()
    numpy_eng = g.Batched2048(64, seed=SEED, rng="numpy")
    numpy_eng.reset()
    with pytest.raises(g.G2048Error, match="numpy-RNG"):
        numpy_eng.play_step(None)
    eng = engine(g, 64)
    before = state(eng)
    net = net_of(g, torch, uniform_case())
    active = torch.ones(64, dtype=torch.int32, device=eng.device).view(torch.uint32)
    act = torch.zeros(64, dtype=torch.uint8, device=eng.device)
    for io, word in ((_lib.NTupleSearchIO(1), b"requests no output"), (_lib.NTupleSearchIO(3, act.data_ptr()), b"depth"),
                     (_lib.NTupleSearchIO(0, act.data_ptr()), b"depth")):
        assert lib.g2048_ntuple_search_active(eng._h, net._ref(eng.device), C.byref(io), active.data_ptr(), None) == -1
        assert word in lib.g2048_last_error()
    io = _lib.NTupleSearchIO(1, act.data_ptr())
    assert lib.g2048_ntuple_search_active(eng._h, None, C.byref(io), active.data_ptr(), None) == -1
    assert lib.g2048_ntuple_search_active(eng._h, net._ref(eng.device), C.byref(io), active.data_ptr() + 2, None) == -1
    assert b"misaligned" in lib.g2048_last_error()
    assert lib.g2048_play_step(eng._h, None, _lib.ACT_U8, None, None) == -1 and b"actions is NULL" in lib.g2048_last_error()
    assert lib.g2048_play_step(eng._h, act.data_ptr(), 7, None, None) == -1 and b"unknown action_dtype" in lib.g2048_last_error()
    after = state(eng)
    assert np.array_equal(before.records, after.records) and before.clock == after.clock and before.stats == after.stats
    close(eng, numpy_eng)


# ------------------------------------------------------------------------------------------------ the masked search
MASKS = ("zeros", "ones", "alternating", "one_zero_in_four")


def mask_of(name, n):
    i = np.arange(n)
    return {"zeros": np.zeros(n, np.uint32), "ones": np.full(n, 0xffffffff, np.uint32) - (i % 3 == 0) * 0xfffffffe,
            "alternating": (i % 2).astype(np.uint32) * 7, "one_zero_in_four": ((i % 4) != (i // 4) % 4).astype(np.uint32) << 31}[name].astype(np.uint32)


def played_engine(g, n, steps=30):
    """n boards some moves into their games (random play), so that the directions differ in legality and value."""
    eng = engine(g, n)
    for _ in range(steps):
        eng.step(None)
    return eng


def assert_masked(torch, eng, net, depth, mask, where):
    n = eng.n_envs
    want = eng.ntuple_search(net, depth)
    active = dev_u32(torch, eng, mask)
    rec, clock = eng.records().clone(), eng.clock
    got = eng.ntuple_search(net, depth, active=active)
    on = torch.from_numpy(mask != 0).to(eng.device)
    assert torch.equal(got.action[on], want.action[on]) and torch.equal(got.value[on], want.value[on]), f"{where}: active rows"
    assert not got.action[~on].any() and bool((got.value[~on] == ILLEGAL).all()), f"{where}: inactive rows"
    # out with one field only; nothing past n is written
    for k, (shape, dtype) in enumerate((((n,), torch.uint8), ((n, 4), torch.int64))):
        buf = torch.full((int(np.prod(shape)) + 512,), 0x5A, dtype=dtype, device=eng.device)
        view = buf[:int(np.prod(shape))].view(shape)
        res = eng.ntuple_search(net, depth, out=g_search(view if k == 0 else None, view if k == 1 else None), active=active)
        assert res[k] is view and res[1 - k] is None and torch.equal(view, got[k]) and bool((buf[int(np.prod(shape)):] == 0x5A).all()), where
    assert torch.equal(eng.records(), rec) and eng.clock == clock and np.array_equal(u32(active), mask)


def g_search(action, value):
    from gym2048_amd.ntuple import NTupleSearch
    return NTupleSearch(action, value)


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("depth, n", [(1, 1), (1, 3), (1, 4), (1, 5), (1, 17), (1, 257), (2, 1), (2, 4), (2, 5)])
def test_search_active(g, torch_cuda, depth, n, mask):
    torch = torch_cuda
    eng = played_engine(g, n)
    m = mask_of(mask, n)
    assert mask in ("zeros", "ones") or n < 4 or (0 < (m != 0).sum() < n)
    assert_masked(torch, eng, net_of(g, torch, uniform_case()), depth, m, f"depth {depth} n={n} {mask}")
    close(eng)


@pytest.mark.parametrize("name", ["staged", "mixed"])
def test_search_active_on_staged_and_mixed_networks(g, torch_cuda, name):
    torch = torch_cuda
    net = net_of(g, torch, staged_case() if name == "staged" else mixed_case())
    for depth, n in ((1, 65), (2, 5)):
        eng = played_engine(g, n, steps=60)
        for mask in ("alternating", "one_zero_in_four"):
            assert_masked(torch, eng, net, depth, mask_of(mask, n), f"{name} depth {depth} {mask}")
        close(eng)


def test_search_active_mask_follows_the_strided_board_index(g, torch_cuda):
    """n * G lanes one pass past the grid cap at depth 1: the boards of the second pass read their own mask entries."""
    torch = torch_cuda
    n = SEARCH_MAX_LANES // SEARCH_GROUP[1] + 17
    assert n == (1 << 20) + 17
    net = g.NTupleNet(((0,),), frac_bits=10)
    net.weights.copy_(torch.from_numpy(np.random.default_rng(41).integers(-(1 << 20), 1 << 20, net.weights.numel()).astype(np.int32))
                      .reshape(net.weights.shape))
    eng = played_engine(g, n, steps=12)
    want = eng.ntuple_search(net, 1)
    mask = np.random.default_rng(42).integers(0, 2, n).astype(np.uint32)
    mask[-17:] = [0, 1] * 8 + [1]
    on = torch.from_numpy(mask != 0).to(eng.device)
    got = eng.ntuple_search(net, 1, active=dev_u32(torch, eng, mask))
    assert len(torch.unique(want.action)) == 4
    assert torch.equal(torch.where(on, want.action, torch.zeros_like(want.action)), got.action)
    assert torch.equal(torch.where(on[:, None], want.value, torch.full_like(want.value, ILLEGAL)), got.value)
    close(eng)


# ------------------------------------------------------------------------------------------------ play_games
def composed_trace(eng, choose, cap=2048):
    """The unlimited trace (as ntuple_play_ref.unlimited's) of rounds of ``choose(eng)`` -> step on the per-move path: as many
    as it takes every board to finish a game, rounded up to a multiple of 8 (``cap`` at the most: asserted)."""
    n, k = eng.n_envs, cap
    rec = lambda: eng.records().cpu().numpy().copy()
    tr = types.SimpleNamespace(n=n, k=k, t0=eng.clock, start=rec(), action=np.zeros((k, n), np.uint8), terminated=np.zeros((k, n), bool),
                               illegal=np.zeros((k, n), bool), gain=np.zeros((k, n), np.int64), after=np.zeros((k, n, 16), np.uint8),
                               terminal=np.zeros((k, n, 16), np.uint8), terminal_score=np.zeros((k, n), np.int64))
    for j in range(k):
        if j % 8 == 0 and tr.terminated[:j].any(axis=0).all():
            return head(tr, j)
        act = choose(eng)
        eng.step(act)
        tr.action[j], tr.terminated[j], tr.illegal[j] = act.cpu().numpy(), eng.terminated.cpu().numpy() != 0, eng.illegal.cpu().numpy() != 0
        tr.gain[j] = np.where(tr.illegal[j], 0, eng.reward.cpu().numpy()).astype(np.int64)
        tr.after[j] = rec()
        done = tr.terminated[j]
        tr.terminal[j][done] = eng.last_records().cpu().numpy()[done]
        tr.terminal_score[j][done] = eng.get_last_scores()[done]
    assert tr.terminated.any(axis=0).all(), f"a first game still runs after {cap} moves"
    return tr


def head(tr, k):
    out = types.SimpleNamespace(**vars(tr))
    out.k = k
    for name in ("action", "terminated", "illegal", "gain", "after", "terminal", "terminal_score"):
        setattr(out, name, getattr(tr, name)[:k])
    return out


def assert_report(report, tr, games, n, first_scores=None):
    """A PlayReport against ``limited`` of a trace with ``games`` games per board."""
    want = pref.limited(tr, np.full(n, games, np.uint32))
    played = int(want.episodes.sum())
    assert report.games == played and report.unfinished == n * games - played
    assert report.mean_score == (want.return_sum / played if played else 0.0)
    assert report.hist == want.hist.astype(np.int64).tolist() and report.moves == want.moves
    assert report.reach == pref.reach_of(want.hist)
    if first_scores is not None:
        assert np.array_equal(report.scores.cpu().numpy(), first_scores)
    else:
        assert report.scores is None
    return want


def first_scores_of(tr):
    """Every board's first final score from a trace in which every board finishes a game."""
    assert tr.terminated.any(axis=0).all()
    first = tr.terminated.argmax(axis=0)
    return tr.terminal_score[first, np.arange(tr.n)].astype(np.int32)


def fresh_pair(g, n):
    """Two engines whose clocks are back at 0, as play_games' reset() will find them (test_gpu_ntuple_play does the same)."""
    a, b = engine(g, n), engine(g, n)
    for e in (a, b):
        e.seed(SEED)
    b.reset()
    return a, b


@pytest.mark.parametrize("depth", [1, 2])
def test_play_games_with_look_ahead(g, torch_cuda, depth):
    torch, n = torch_cuda, 64
    net = net_of(g, torch, uniform_case())
    a, b = fresh_pair(g, n)
    tr = composed_trace(b, lambda e: e.ntuple_search(net, depth).action)
    K, cut = tr.k, max(8, tr.k // 16 * 8)
    by_cut = head(tr, cut).terminated.sum(axis=0)
    assert by_cut.sum() > 0 and (by_cut < 2).any(), "inputs: at the cut some games are over and some are owed"
    report = g.play_games(a, net, games=1, chunk=K, depth=depth)
    want = assert_report(report, tr, 1, n, first_scores_of(tr))
    assert report.games == n and report.unfinished == 0 and want.played.sum() < K * n     # boards rested
    # two games per board, cut short: what is over is reported, the rest is owed
    a.seed(SEED)
    short = g.play_games(a, net, games=2, chunk=8, max_steps=cut, depth=depth)
    want = assert_report(short, head(tr, cut), 2, n)
    assert 0 < short.unfinished < 2 * n and short.unfinished == int(want.games_left.sum())
    close(a, b)


def test_play_games_depth_0_is_the_fused_loop(g, torch_cuda):
    """The default path launches what it launched: ntuple_play in chunks, the report of test_gpu_ntuple_play's reference."""
    torch, n = torch_cuda, 64
    case = uniform_case(T=1)
    score, top, length = pref.first_games(n, SEED, case.rnet, cap=2000)
    assert (score >= 0).all()
    net = net_of(g, torch, case)
    eng = engine(g, n)
    eng.seed(SEED)
    calls = []
    play, step = eng.ntuple_play, eng.play_step
    eng.ntuple_play = lambda *a, **kw: (calls.append("play"), play(*a, **kw))[1]
    eng.play_step = lambda *a, **kw: (calls.append("step"), step(*a, **kw))[1]
    for kw in ({}, dict(depth=0), dict(depth=0, player=None)):
        eng.seed(SEED)
        report = g.play_games(eng, net, 1, 64, None, **kw)
        assert np.array_equal(report.scores.cpu().numpy(), score) and report.mean_score == int(score.sum()) / n
        assert report.hist == np.bincount(top, minlength=32).tolist() and report.moves == int(length.sum()) and report.unfinished == 0
    assert calls and set(calls) == {"play"}
    close(eng)


def test_play_games_with_the_random_player_matches_the_cpu_reference(g, torch_cuda):
    torch, n, K = torch_cuda, 64, 96
    o = pref.start_of(n, SEED)
    table = np.zeros((K, n), np.uint8)
    eng = engine(g, n)
    eng.seed(SEED)
    eng.reset()
    table[:] = eng.random_actions(K).cpu().numpy()                   # the synthetic policy of transactions 2 .. K + 1
    tr = psh.unlimited(o, table)
    assert tr.terminated.any(axis=0).all()
    eng.seed(SEED)
    report = g.play_games(eng, None, games=1, chunk=K, player=lambda e, a: e.random_actions(1, out=a.view(1, -1)))
    assert_report(report, tr, 1, n, first_scores_of(tr))
    eng.seed(SEED)
    two = g.play_games(eng, None, games=2, chunk=32, max_steps=K, player=lambda e, a: e.random_actions(1, out=a.view(1, -1)))
    assert_report(two, tr, 2, n)
    close(eng)


def test_play_games_with_the_expectimax_player_matches_the_composition(g, torch_cuda):
    torch, n = torch_cuda, 64
    a, b = fresh_pair(g, n)
    b.set_max_tile(32)
    a.set_max_tile(32)                                               # short games: a game ends on its first 32
    tr = composed_trace(b, lambda e: e.expectimax(depth=1).action)
    K = tr.k

    def player(e, actions):
        e.expectimax(depth=1, out=g.Search(actions, None))

    report = g.play_games(a, None, games=1, chunk=K, player=player)
    assert_report(report, tr, 1, n, first_scores_of(tr))
    assert max(k for k, c in enumerate(report.hist) if c) == 5
    close(a, b)
