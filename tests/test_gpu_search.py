"""GPU: the expectimax kernels (g2048_expectimax, g2048_expectimax_plain) equal the host build of the same header bit for
bit, touch nothing of the engine, honour ``out`` and the current stream, and play far better than the random policy."""
import numpy as np
import pytest

import search_ref as ref
from test_search_host import build_search_check, host_search, random_boards, trajectory_boards

pytestmark = pytest.mark.gpu

ODD_W = (12345, 7, 65535, 3)


@pytest.fixture(scope="module")
def hs(tmp_path_factory):
    return build_search_check(tmp_path_factory.mktemp("search_check_gpu"))


@pytest.fixture(scope="module")
def g(torch_cuda):
    import gym2048_amd
    return gym2048_amd


def device_search(g, torch, boards, depth, w=None):
    s = g.expectimax(torch.as_tensor(np.ascontiguousarray(boards)).to("cuda:0"), depth, w)
    torch.cuda.synchronize()
    return s.action.cpu().numpy(), s.value.cpu().numpy()


def assert_same(dev, host):
    bad = np.nonzero((dev[0] != host[0]) | (dev[1] != host[1]).any(1))[0]
    assert len(bad) == 0, f"{len(bad)} boards differ, first index {bad[0]}: {dev[0][bad[0]]} {dev[1][bad[0]]} vs " \
                          f"{host[0][bad[0]]} {host[1][bad[0]]}"


@pytest.mark.parametrize("depth,n", [(1, 1 << 16), (1, (1 << 16) - 37), (2, 4096), (2, 4096 - 13), (3, 64), (3, 61)])
def test_device_equals_host(g, torch_cuda, hs, depth, n):
    boards = random_boards(n, 10 + depth)
    if depth >= 2:  # mid-game boards from the golden trajectories for half of them
        traj = trajectory_boards(every=3)
        boards[::2] = traj[np.random.default_rng(depth).integers(0, len(traj), len(boards[::2]))]
    for w in (None, ODD_W):
        dev = device_search(g, torch_cuda, boards, depth, w)
        assert_same(dev, host_search(hs, boards, depth, ref.DEFAULT_WEIGHTS if w is None else w))


def test_device_hand_cases_and_extremes(g, torch_cuda, hs):
    for name, (board, depth, w, expected) in ref.HAND_CASES.items():
        dev = device_search(g, torch_cuda, board[None], depth, w)
        assert_same(dev, ref.search_batch(board[None], depth, w))
        if expected is not None:
            assert dev[0][0] == expected, name
    # exponents up to 31 (mod 32 input) at the largest weights; the input's high bits are ignored
    boards = random_boards(3000, 20, max_exp=31)
    wmax = (1 << 24, 65535, 65535, 65535)
    dev = device_search(g, torch_cuda, boards, 1, wmax)
    assert_same(dev, host_search(hs, boards, 1, wmax))
    assert_same(device_search(g, torch_cuda, boards | np.where(boards > 0, 32, 0).astype(np.uint8), 1, wmax), dev)


def test_engine_form_equals_plain_and_touches_nothing(g, torch_cuda):
    torch = torch_cuda
    for rng in ("philox", "numpy"):
        eng = g.Batched2048(3000, seed=5, rng=rng)
        try:
            eng.reset()
            eng.rollout_random(40)
            torch.cuda.synchronize()
            rec, clock, stats = eng.records().clone(), eng.clock, eng.episode_stats()
            planes = eng.get_numpy_rng() if rng == "numpy" else None
            for depth in (1, 2):
                s = eng.expectimax(depth)
                p = g.expectimax(torch.as_tensor(eng.get_boards().reshape(-1, 16)).cuda(), depth)
                torch.cuda.synchronize()
                assert torch.equal(s.action, p.action) and torch.equal(s.value, p.value)
            assert torch.equal(eng.records(), rec)
            assert eng.clock == clock and eng.episode_stats() == stats
            if planes is not None:
                assert np.array_equal(eng.get_numpy_rng(), planes)
        finally:
            eng.close()


def test_out_reuse_and_stream_order(g, torch_cuda):
    torch = torch_cuda
    boards = torch.as_tensor(random_boards(5000, 30)).cuda()
    want = g.expectimax(boards, 1)
    out = g.Search(torch.full((5000,), 7, dtype=torch.uint8, device="cuda"), torch.zeros((5000, 4), dtype=torch.int32, device="cuda"))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        src = torch.empty_like(boards)
        torch.cuda._sleep(1 << 20)           # the copy below lands late: a search on another stream would see garbage
        src.copy_(boards)
        got = g.expectimax(src, 1, out=out)
    torch.cuda.synchronize()
    assert got is out or (got.action is out.action and got.value is out.value)
    assert torch.equal(out.action, want.action) and torch.equal(out.value, want.value)
    # a None field is not written
    only = g.Search(None, torch.full((5000, 4), -5, dtype=torch.int32, device="cuda"))
    g.expectimax(boards, 2, out=only)
    acts = torch.full((5000,), 9, dtype=torch.uint8, device="cuda")
    g.expectimax(boards, 2, out=g.Search(acts, None))
    torch.cuda.synchronize()
    assert only.action is None and torch.equal(acts, g.expectimax(boards, 2).action)
    assert torch.equal(only.value, g.expectimax(boards, 2).value)


def play(g, torch, n, seed, policy, cap=5000):
    """Final score of every board's first game (numpy-RNG mode), and whether any searched move was illegal."""
    eng = g.Batched2048(n, seed=seed, rng="numpy")
    gen = torch.Generator(device="cuda").manual_seed(seed)
    first = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    illegal = False
    try:
        eng.reset()
        for _ in range(cap):
            if policy == "search":
                a = eng.expectimax(1).action
            else:
                a = torch.randint(0, 4, (n,), generator=gen, device="cuda", dtype=torch.uint8)
            eng.step(a)
            live = first < 0
            if policy == "search":
                illegal |= bool((eng.illegal.bool() & live).any())
            ended = eng.terminated.bool() & live
            if bool(ended.any()):
                first[ended] = eng.last_scores().to(torch.int64)[ended]
            if not bool((first < 0).any()):
                break
        return first.cpu().numpy(), illegal
    finally:
        eng.close()


def test_depth1_plays_well(g, torch_cuda):
    n, seed = 512, 2048
    searched, illegal = play(g, torch_cuda, n, seed, "search")
    rand, _ = play(g, torch_cuda, n, seed, "random")
    assert not illegal, "the search picked an illegal move while a legal one existed"
    assert (searched >= 0).all() and (rand >= 0).all(), "a game outlived the 5 000-move cap"
    assert searched.mean() >= 10 * rand.mean(), (searched.mean(), rand.mean())


def test_record_search(g, torch_cuda, tmp_path):
    from gym2048_amd.batched import values_to_exp
    from gym2048_amd.transitions import Transitions
    torch = torch_cuda
    n, k = 64, 24
    eng = g.Batched2048(n, seed=9)
    try:
        eng.reset()
        tr = Transitions.record_search(eng, k, depth=2, weights=ODD_W)
    finally:
        eng.close()
    assert tr.size() == n * k
    boards = values_to_exp(tr.x).reshape(-1, 16).astype(np.uint8)
    s = g.expectimax(torch.as_tensor(boards).cuda(), 2, ODD_W)
    assert np.array_equal(tr.action.reshape(-1), s.action.cpu().numpy())
    # env-major rows: within an env, next_board is the following row's board unless the step ended the episode
    nxt = values_to_exp(tr.next_x).reshape(n, k, 16)
    cur = boards.reshape(n, k, 16)
    done = tr.done.reshape(n, k)
    assert np.array_equal(nxt[:, :-1][~done[:, :-1]], cur[:, 1:][~done[:, :-1]])
    path = tmp_path / "bc.csv"
    tr.export_csv(str(path))
    back = Transitions.import_csv(str(path))
    for f in ("x", "action", "reward", "next_x", "done"):
        assert np.array_equal(getattr(back, f), getattr(tr, f)), f
    assert back.to_csv_text() == tr.to_csv_text()
