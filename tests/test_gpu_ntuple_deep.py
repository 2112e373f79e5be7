"""GPU: the n-tuple deep search kernel (g2048_ntuple_deep_search), one workgroup per board.  Depth 3
against the pure-Python reference on near-full boards; depth 2 against the existing g2048_ntuple_search, bit for bit, on every
kind of board and network; depth 3 on wide boards against the definition composed from depth-2 calls of the existing kernel
(ntuple_deep_helpers.compose_depth3); the mask, the grid cap, the engine's state, and the game report of DeepPlayer.  Every
test shows from the reference or the definition (never from the code under test) that its input reaches the edge it names."""
import numpy as np
import pytest

import ntuple_search_ref as sref
from analysis_helpers import ONE_LEGAL, TERMINAL, assert_rows_periodic, g, mixed_boards, tiled  # noqa: F401 (g: fixture)
from ntuple_deep_helpers import (ILLEGAL, composed_game, compose_depth3, dev, dev_u32, device_net, engine_with, mixed_net, near_full,
                                 staged_net, to_np)
from ntuple_helpers import TUPLES_2x6, TUPLES_8x4, random_net
from ntuple_search_helpers import PAIR_ONLY, WIDE_FANS, assert_search_equal

pytestmark = pytest.mark.gpu
MAX_WORKGROUPS = (1 << 24) // 256      # kSearchMaxLanes / kBlock (g2048_kernels.hip): the grid cap of the deep search kernel


def named_nets():
    return {"1x4": random_net(TUPLES_8x4[:1], 41), "2x6": random_net(TUPLES_2x6, 42), "8x4": random_net(TUPLES_8x4, 43),
            "mixed": mixed_net(), "staged": staged_net()}


_named = {}


def named_net(name):
    if not _named:
        _named.update(named_nets())
    return _named[name]


# ------------------------------------------------------------------------------------------------ depth 3, the reference
def test_depth_3_equals_the_reference(g, torch_cuda):
    torch = torch_cuda
    boards, rnet, want3, want2, trace = near_full(2)
    assert trace.chance > 4000 and trace.negative_inexact > 200 and trace.terminal_children > 30
    assert (want3[0] != want2[0]).any() and len(boards) == 6
    net, d = device_net(g, rnet), dev(torch, boards)
    assert_search_equal(to_np(net.deep_search(d)), want3, boards, "plain, depth 3 by default")
    assert_search_equal(to_np(net.deep_search(d.view(-1, 4, 4), 3)), want3, boards, "plain [n, 4, 4]")
    assert_search_equal(to_np(net.deep_search(d, 2)), want2, boards, "plain, depth 2")
    eng = engine_with(g, boards)
    try:
        assert bool((eng.records()[:, 8:] > 31).any())
        assert_search_equal(to_np(eng.ntuple_deep_search(net)), want3, boards, "engine")
        assert_search_equal(to_np(eng.ntuple_deep_search(net, 2)), want2, boards, "engine, depth 2")
    finally:
        eng.close()


def test_depth_3_of_one_board(g, torch_cuda):
    torch = torch_cuda
    boards, rnet, want3, _, _ = near_full(2)
    net = device_net(g, rnet)
    for i in (0, 5):
        one = boards[i:i + 1]
        assert_search_equal(to_np(net.deep_search(dev(torch, one), 3)), (want3[0][i:i + 1], want3[1][i:i + 1]), one, f"plain, board {i}")
    eng = engine_with(g, boards[2:3])
    try:
        assert_search_equal(to_np(eng.ntuple_deep_search(net, 3)), (want3[0][2:3], want3[1][2:3]), boards[2:3], "engine, n = 1")
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ depth 2, the existing kernel
def depth2_boards():
    return np.concatenate([mixed_boards(257, 44), ONE_LEGAL, TERMINAL, PAIR_ONLY, WIDE_FANS])


@pytest.mark.parametrize("name", ["1x4", "2x6", "8x4", "mixed", "staged"])
def test_depth_2_equals_the_existing_search(g, torch_cuda, name):
    torch = torch_cuda
    boards = depth2_boards()
    empties = (boards == 0).sum(1)
    assert len(boards) == 270 and empties.min() == 0 and empties.max() == 16 and (empties == 15).any(), "inputs: full, one-tile and empty boards"
    rnet = named_net(name)
    assert len(rnet.tuples) == {"1x4": 1, "2x6": 2, "8x4": 8, "mixed": 4, "staged": 2}[name]
    net, d = device_net(g, rnet), dev(torch, boards)
    want = net.search(d, 2)
    legal = want.value != ILLEGAL
    assert bool(legal.any()) and bool((~legal).any()) and len(set(want.action.tolist())) == 4
    got = net.deep_search(d, 2)
    assert_search_equal(to_np(got), to_np(want), boards, f"{name}, plain")
    eng = engine_with(g, boards)
    try:
        assert_search_equal(to_np(eng.ntuple_deep_search(net, 2)), to_np(want), boards, f"{name}, engine")
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ depth 3, composed
@pytest.mark.parametrize("name", ["1x4", "2x6", "mixed", "staged"])
def test_depth_3_equals_the_composition_of_depth_2_calls(g, torch_cuda, name):
    """value[d] = (g << F) + (sum of w * S_2(child)) // (10 E) with S_2 from g2048_ntuple_search_plain at depth 2: the oracle
    needs no slow reference, so it takes wide boards."""
    torch = torch_cuda
    boards = {"1x4": WIDE_FANS, "2x6": np.concatenate([mixed_boards(63, 45), PAIR_ONLY]),
              "mixed": np.concatenate([mixed_boards(15, 46), PAIR_ONLY]), "staged": np.concatenate([mixed_boards(15, 47), PAIR_ONLY])}[name]
    rnet = named_net(name)
    net = device_net(g, rnet)
    want, widest, dead = compose_depth3(boards, rnet.frac_bits, lambda kids: net.search(dev(torch, kids), 2).value.cpu().numpy())
    if name == "1x4":
        assert widest == 30 and len(boards) == 10, "inputs: a direction with 30 level-1 items"
    else:
        assert dead >= 1, "inputs: a child with no legal move"
    legal = want[1] != ILLEGAL
    assert legal.any() and (np.abs(want[1][legal]) < 1 << 50).all()
    assert_search_equal(to_np(net.deep_search(dev(torch, boards), 3)), want, boards, name)


# ------------------------------------------------------------------------------------------------ the mask, the outputs
def test_mask(g, torch_cuda):
    torch = torch_cuda
    rnet = named_net("1x4")
    net = device_net(g, rnet)
    boards = np.concatenate([near_full(2)[0][:4], PAIR_ONLY])
    for n in (1, 3, 5):
        b = boards[:n]
        eng = engine_with(g, b)
        try:
            for depth in (2, 3):
                want = eng.ntuple_deep_search(net, depth)
                assert bool((want.value != ILLEGAL).any(1).all()), "inputs: every board has a legal move"
                on = eng.ntuple_deep_search(net, depth, active=dev_u32(torch, np.full(n, 7)))
                assert torch.equal(on.action, want.action) and torch.equal(on.value, want.value)
                off = eng.ntuple_deep_search(net, depth, active=dev_u32(torch, np.zeros(n)))
                assert bool((off.action == 0).all()) and bool((off.value == ILLEGAL).all())
                mask = np.arange(n) % 2 == 0
                alt = eng.ntuple_deep_search(net, depth, active=dev_u32(torch, np.where(mask, 1 << 31, 0)))
                m = torch.from_numpy(mask).to("cuda:0")
                assert torch.equal(alt.action[m], want.action[m]) and torch.equal(alt.value[m], want.value[m])
                assert bool((alt.action[~m] == 0).all()) and bool((alt.value[~m] == ILLEGAL).all())
        finally:
            eng.close()


def test_out_fields_left_none_are_not_written(g, torch_cuda):
    torch = torch_cuda
    boards, rnet, want3, _, _ = near_full(2)
    n = len(boards)
    net, d = device_net(g, rnet), dev(torch, boards)
    eng = engine_with(g, boards)
    try:
        for form in ("plain", "engine", "masked"):
            act = torch.full((n + 512,), 0x5A, dtype=torch.uint8, device="cuda")
            val = torch.full((4 * n + 512,), 0x5A5A, dtype=torch.int64, device="cuda")
            call = {"plain": lambda out: net.deep_search(d, 3, out=out), "engine": lambda out: eng.ntuple_deep_search(net, 3, out=out),
                    "masked": lambda out: eng.ntuple_deep_search(net, 3, out=out, active=dev_u32(torch, np.ones(n)))}[form]
            res = call(g.NTupleSearch(act[:n], None))
            assert res.value is None and res.action is not None and np.array_equal(res.action.cpu().numpy(), want3[0]), form
            assert bool((act[n:] == 0x5A).all()) and bool((val == 0x5A5A).all()), form
            act.fill_(0x5A)
            res = call(g.NTupleSearch(None, val[:4 * n].view(n, 4)))
            assert res.action is None and np.array_equal(res.value.cpu().numpy(), want3[1]), form
            assert bool((val[4 * n:] == 0x5A5A).all()) and bool((act == 0x5A).all()), form
        with pytest.raises(ValueError, match="no output"):
            net.deep_search(d, out=g.NTupleSearch(None, None))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ the grid cap
def test_workgroups_stride_past_the_grid_cap(g, torch_cuda):
    """n = 65 536 + 3 boards: the last three are reached by the first three workgroups' second pass.  Boards that cost almost
    nothing (no move, one move, two moves onto one empty cell), depth 2 against the existing kernel."""
    torch = torch_cuda
    base = np.concatenate([TERMINAL, ONE_LEGAL, PAIR_ONLY])
    n = MAX_WORKGROUPS + 3
    assert n % len(base) != 0 and n > MAX_WORKGROUPS
    rnet = named_net("1x4")
    net = device_net(g, rnet)
    want = net.search(dev(torch, base), 2)
    assert_search_equal(to_np(want), sref.search_batch(base, 2, rnet), base, "base")
    d = tiled(torch, base, n).contiguous()
    got = net.deep_search(d, 2)
    for k in range(2):
        assert_rows_periodic(torch, got[k], want[k], 1 << 20)
    last = net.search(d[-3:].contiguous(), 2)
    assert torch.equal(got.action[-3:], last.action) and torch.equal(got.value[-3:], last.value)
    assert len({tuple(r) for r in got.value[-3:].cpu().numpy().tolist()}) == 3, "the last three boards differ from one another"


# ------------------------------------------------------------------------------------------------ the engine is left alone
def test_the_engine_s_state_is_untouched(g, torch_cuda):
    torch = torch_cuda
    rnet = named_net("1x4")
    net = device_net(g, rnet)
    eng = g.Batched2048(64, seed=5)
    try:
        eng.reset()
        for _ in range(40):
            eng.step(None)
        torch.cuda.synchronize()
        rec, clock, stats, replays = eng.records().clone(), eng.clock, eng.episode_stats(), eng.graph_replays
        assert eng.last_records_enabled and stats["episodes"] >= 0
        last = eng.last_records().clone()
        mask = dev_u32(torch, np.arange(64) % 3 != 0)
        eng.ntuple_deep_search(net, 2)
        eng.ntuple_deep_search(net, 2, active=mask)
        eng.ntuple_deep_search(net, 3, active=dev_u32(torch, (np.arange(64) < 4)))
        assert torch.equal(eng.records(), rec) and eng.clock == clock and eng.episode_stats() == stats and eng.graph_replays == replays
        assert torch.equal(eng.last_records(), last)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ games
def report_fields(r):
    return r.games, r.unfinished, r.mean_score, r.hist, r.reach, r.moves


def test_play_games_with_the_deep_player_is_the_composition(g, torch_cuda):
    """play_games(player=DeepPlayer(net)) against ntuple_deep_search(active=games left) -> play_step, call by call, on a second
    engine with the same seed: eight moves of four fresh boards at depth 3."""
    torch = torch_cuda
    rnet = named_net("1x4")
    net = device_net(g, rnet)
    a, b = g.Batched2048(4, seed=11), g.Batched2048(4, seed=11)
    try:
        report = g.play_games(a, net, games=1, chunk=4, max_steps=8, player=g.DeepPlayer(net))
        want = composed_game(torch, b, net, 3, 8)
        assert len({tuple(r) for r in want.actions.T.tolist()}) > 1, "inputs: the boards do not all play the same moves"
        assert report.games == want.played and report.unfinished == 4 - want.played and report.moves == want.moves == 32
        assert report.hist == want.hist and report.mean_score == (want.return_sum / want.played if want.played else 0.0)
        assert torch.equal(a.records(), b.records()) and a.clock == b.clock and a.episode_stats() == b.episode_stats()
    finally:
        a.close(), b.close()


def test_deep_player_at_depth_2_gives_the_report_of_depth_2(g, torch_cuda):
    rnet = named_net("1x4")
    net = device_net(g, rnet)
    a, b = g.Batched2048(16, seed=12), g.Batched2048(16, seed=12)
    try:
        want = g.play_games(a, net, games=1, chunk=8, max_steps=48, depth=2)
        got = g.play_games(b, net, games=1, chunk=8, max_steps=48, player=g.DeepPlayer(net, depth=2))
        assert want.moves > 16 * 8 and report_fields(got) == report_fields(want)
        assert (got.scores is None) == (want.scores is None) and (want.scores is None or bool((got.scores == want.scores).all()))
        assert a.clock == b.clock and a.episode_stats() == b.episode_stats() and bool((a.records() == b.records()).all())
    finally:
        a.close(), b.close()
