"""GPU: game reports with tile-downgrading (play_games(..., downgrade=), DowngradedPlayer) against the
hand-written loop each of them stands for, and optimistic initialisation (NTupleNet.fill_value, init_value).  64 boards, one
game each, a rule that is at work from the 32 tile on, so that the short games of a random network use it.  These tests fail
without the feature: ``play_games`` takes no ``downgrade`` and the network has no ``fill_value``."""
import numpy as np
import pytest

from downgrade_helpers import net_of, small_case

pytestmark = pytest.mark.gpu
SEED, N, CHUNK = 77, 64, 64


@pytest.fixture(scope="module")
def g(torch_cuda):
    import gym2048_amd
    return gym2048_amd


def hand_loop(torch, g, eng, rule, move):
    """play_games's report by hand: reset, one game per board, ``move(boards, act)`` fills the actions from the translated
    boards; (games, mean score, hist, moves, scores)."""
    n, d = eng.n_envs, eng.device
    eng.reset()
    left = torch.ones(n, dtype=torch.int32, device=d).view(torch.uint32)
    hist = torch.zeros(32, dtype=torch.int64, device=d).view(torch.uint64)
    moves = torch.zeros(1, dtype=torch.int64, device=d).view(torch.uint64)
    low = g.Downgraded(torch.empty((n, 16), dtype=torch.uint8, device=d), torch.empty(n, dtype=torch.uint8, device=d))
    act = torch.empty(n, dtype=torch.uint8, device=d)
    before, at_work = eng.episode_stats(), 0
    while bool(left.view(torch.int32).any()):
        for _ in range(CHUNK):
            eng.downgraded_boards(rule, active=left, out=low)
            at_work += int(((low.missing != 0) & (low.missing != 0xff)).sum())
            move(low.boards, act)
            eng.play_step(act, games_left=left, hist=hist, moves=moves)
    after = eng.episode_stats()
    games = after["episodes"] - before["episodes"]
    assert at_work >= 100, "the rule was at work"
    return games, (after["return_sum"] - before["return_sum"]) / games, hist.view(torch.int64).tolist(), int(moves.view(torch.int64)[0]), eng.last_scores()


@pytest.mark.parametrize("player", ["greedy", "depth1", "deep2"])
def test_play_games_is_the_hand_written_loop(g, torch_cuda, player):
    torch = torch_cuda
    from gym2048_amd.ntuple import NTupleEval, NTupleSearch
    net, rule = net_of(g, torch, small_case("staged", 4)), g.Downgrade(32, 16)
    eng = g.Batched2048(N, seed=SEED)
    eng.seed(SEED)
    if player == "greedy":
        report = g.play_games(eng, net, games=1, chunk=CHUNK, downgrade=rule)
        move = lambda boards, act: net.evaluate(boards, out=NTupleEval(None, act, None, None, None))      # noqa: E731
    elif player == "depth1":
        report = g.play_games(eng, net, games=1, chunk=CHUNK, depth=1, downgrade=rule)
        move = lambda boards, act: net.search(boards, 1, out=NTupleSearch(act, None))                     # noqa: E731
    else:
        report = g.play_games(eng, None, games=1, chunk=CHUNK, player=g.DowngradedPlayer(g.DeepPlayer(net, 2), rule))
        move = lambda boards, act: net.deep_search(boards, 2, out=NTupleSearch(act, None))                # noqa: E731
    eng.seed(SEED)
    games, mean, hist, moves, scores = hand_loop(torch, g, eng, rule, move)
    assert report.games == games == N and report.unfinished == 0
    assert report.mean_score == mean and report.hist == hist and report.moves == moves
    assert report.reach == {tile: sum(hist[tile.bit_length() - 1:]) / N for tile in (2048, 4096, 8192, 16384, 32768)}
    assert torch.equal(report.scores, scores)
    eng.close()


def test_the_other_wrapped_players_run_the_plain_search_of_translated_boards(g, torch_cuda):
    """AdaptivePlayer and ReducedPlayer under DowngradedPlayer: one move's actions are those of the plain search of
    downgraded_boards, and a resting board gets action 0."""
    torch = torch_cuda
    from gym2048_amd.ntuple import schedule_by_empties
    net, rule = net_of(g, torch, small_case("uniform", 3)), g.Downgrade(32, 16)
    eng = g.Batched2048(N, seed=SEED)
    eng.reset()
    rs = np.random.default_rng(6)
    eng.set_boards(np.where(rs.random((N, 16)) < 0.3, 0, rs.integers(1, 9, (N, 16))).astype(np.uint8))
    active = torch.ones(N, dtype=torch.int32, device=eng.device).view(torch.uint32)
    active.view(torch.int32)[::5] = 0
    low = eng.downgraded_boards(rule, active=active)
    assert ((low.missing != 0) & (low.missing != 0xff)).sum() >= 10
    sched = schedule_by_empties({4: 2}, 1)      # 2-ply up to four empty cells, 1-ply above
    for wrapped, want in ((g.AdaptivePlayer(net, sched), lambda: net.adaptive_search(low.boards, sched).action),
                          (g.ReducedPlayer(net, sched, 1), lambda: net.reduced_search(low.boards, sched, 1).action)):
        act = torch.full((N,), 9, dtype=torch.uint8, device=eng.device)
        g.DowngradedPlayer(wrapped, rule)(eng, act, active=active)
        assert torch.equal(act, want()) and not act[::5].any()
    eng.close()


@pytest.mark.parametrize("family, T", [("uniform", 5), ("mixed", 8), ("staged", 4)])
def test_fill_value(g, torch_cuda, family, T):
    """V of every board is the constant: 8 T times the weight floor((score << F) / (8 T)), whatever the board, its stage or the
    lengths of the tuples."""
    torch = torch_cuda
    case = small_case(family, T)
    net = g.NTupleNet(case.tuples, frac_bits=10, stages=case.stages, mixed=True, init_value=50000)
    weight = (50000 << 10) // (8 * T)
    assert bool((net.weights == weight).all())
    rs = np.random.default_rng(7)
    cells = np.where(rs.random((500, 16)) < 0.3, 0, rs.integers(1, 18, (500, 16)))
    cells[:100], cells[100:200] = cells[:100] % 4, cells[100:200] % 6     # up to 8, up to 32: the two early stages of a staged case
    boards = torch.from_numpy(cells.astype(np.uint8)).to(net.device)
    assert net.stages is None or len(set(net.stage(boards).tolist())) == 3
    assert bool((net.values(boards) == 8 * T * weight).all()) and 0 <= (50000 << 10) - 8 * T * weight < 8 * T
    net.fill_value(-3)
    assert bool((net.values(boards) == 8 * T * ((-3 << 10) // (8 * T))).all())
    with pytest.raises(ValueError, match="does not fit in int32"):
        net.fill_value(1 << 40)
    assert bool((net.weights == (-3 << 10) // (8 * T)).all())
