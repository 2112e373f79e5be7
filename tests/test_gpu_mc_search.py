"""GPU: the Monte-Carlo search kernel (g2048_mc_search, g2048_mc_search_plain) equals the host build of the same header
bit for bit, follows the board-index rule across forms, shards and grid passes, touches nothing of the engine, honours
``out`` and the current stream, and plays far better than the random policy.

Figures measured on the MI355X: profiles/r09_mc_probe.txt and the strength test's docstring."""
import numpy as np
import pytest

from analysis_helpers import (ONE_LEGAL, SEARCH_MAX_LANES, SEED, TERMINAL, WAVE_ROLLOUTS, g, high_boards, hm, host_mc,  # noqa: F401
                              legal_count, mixed_boards, play, random_boards, random_policy)  # (g, hm: fixtures)

pytestmark = pytest.mark.gpu


def to_np(s):
    return tuple(None if t is None else t.cpu().numpy() for t in s)


def device_mc(g, torch, boards, R, L, seed=SEED, index_offset=0):
    s = g.mc_search(torch.as_tensor(np.ascontiguousarray(boards)).to("cuda:0"), R, L, seed, index_offset)
    torch.cuda.synchronize()
    return to_np(s)


def assert_same(dev, host, where=""):
    bad = np.nonzero((dev[0] != host[0]) | (dev[1] != host[1]).any(1) | (dev[2] != host[2]).any(1))[0]
    assert len(bad) == 0, f"{where}: {len(bad)} boards differ, first index {bad[0]}: {[x[bad[0]].tolist() for x in dev]} vs " \
                          f"{[x[bad[0]].tolist() for x in host]}"


# R below, equal to and above the lanes per direction of the 16-lane form (4); 31 / 32 straddle the switch to the
# 64-lane form, whose 16 lanes per direction 67 does not divide; L from 1 to "to the end of the game"
@pytest.mark.parametrize("R,L,n", [(1, 1, 4096), (3, 12, 4096 - 13), (4, 40, 2048), (5, 8, 2048), (31, 20, 512), (32, 20, 512),
                                   (67, 30, 301), (8, 65535, 512), (64, 65535, 64)])
def test_device_equals_host(g, torch_cuda, hm, R, L, n):
    boards = mixed_boards(n, 10 + R)
    host = host_mc(hm, boards, R, L, index_offset=12345)
    assert_same(device_mc(g, torch_cuda, boards, R, L, index_offset=12345), host, (R, L))
    played = host[2][host[2] >= 0]
    if L == 65535:   # most playouts end terminal: none can have reached the cap
        assert played.max() < R * L and played.mean() > 20 * R
    if L <= 12:      # and here most hit the cap
        assert (played == R * L).mean() > 0.5


def test_high_boards_and_hand_cases(g, torch_cuda, hm):
    """Exponents 26..31: a direction's sum passes 2^32 (the 64-bit partial sums must meet whole in the shuffles); boards
    with one and with no legal move; exponents are read mod 32."""
    boards = high_boards(256, 40, (2, 6))
    for R, L in ((8, 30), (40, 30)):
        host = host_mc(hm, boards, R, L)
        assert host[1].max() >= 1 << 32
        assert_same(device_mc(g, torch_cuda, boards, R, L), host, (R, L))
    hand = np.concatenate([ONE_LEGAL, TERMINAL, ONE_LEGAL, TERMINAL, random_boards(60, 41)])
    assert legal_count(hand[:2]).tolist() == [1, 0]
    for R in (3, 64):
        dev = device_mc(g, torch_cuda, hand, R, 50)
        assert_same(dev, host_mc(hm, hand, R, 50), R)
        assert dev[0][1] == 0 and (dev[1][1] == -1).all() and (dev[2][1] == -1).all() and dev[0][0] == 2
    low = random_boards(500, 42, max_exp=17)
    assert_same(device_mc(g, torch_cuda, low | np.where(low > 0, 32, 0).astype(np.uint8), 5, 20), host_mc(hm, low, 5, 20), "mod 32")


def test_engine_form_index_rule_and_touches_nothing(g, torch_cuda, hm):
    """Engine form == plain form at index_offset = board_offset == host; two shards == the unsharded batch; the engine's
    state blob, clock and graph replay count are the same before and after, in both RNG modes."""
    torch = torch_cuda
    n, off = 3000, 70000
    for rng in ("philox", "numpy"):
        eng = g.Batched2048(n, seed=5, rng=rng, board_offset=off)
        try:
            eng.reset()
            eng.rollout_random(40)
            torch.cuda.synchronize()
            state, clock, replays, stats = eng.state_dict(), eng.clock, eng.graph_replays, eng.episode_stats()
            rec = eng.records().clone()
            cells = eng.get_boards().reshape(-1, 16)
            dev = torch.as_tensor(cells).cuda()
            for R, L in ((6, 25), (33, 15)):
                s = eng.mc_search(R, L, seed=SEED)
                p = g.mc_search(dev, R, L, SEED, index_offset=off)
                torch.cuda.synchronize()
                for a, b in zip(s, p):
                    assert torch.equal(a, b), (rng, R)
                assert_same(to_np(s), host_mc(hm, cells, R, L, index_offset=off), (rng, R))
                # the index is part of the stream: the same boards at another offset give other values
                q = g.mc_search(dev, R, L, SEED, index_offset=off + 1)
                assert not torch.equal(q.value, p.value)
                # two shards of the batch
                cut = 1111
                lo = g.mc_search(dev[:cut].contiguous(), R, L, SEED, index_offset=off)
                hi = g.mc_search(dev[cut:].contiguous(), R, L, SEED, index_offset=off + cut)
                for k in range(3):
                    assert torch.equal(torch.cat([lo[k], hi[k]]), p[k]), (rng, R, k)
                # another seed changes the values, the same seed repeats them
                other = eng.mc_search(R, L, seed=SEED ^ (1 << 40))
                again = eng.mc_search(R, L, seed=SEED)
                assert not torch.equal(other.value, s.value) and torch.equal(again.value, s.value)
                assert torch.equal(again.steps, s.steps) and torch.equal(again.action, s.action)
            torch.cuda.synchronize()
            assert torch.equal(eng.records(), rec)
            assert eng.clock == clock and eng.graph_replays == replays and eng.episode_stats() == stats
            after = eng.state_dict()
            assert after.keys() == state.keys()
            for k in state:
                x, y = state[k], after[k]
                same = torch.equal(x, y) if isinstance(x, torch.Tensor) else (np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y)
                assert same, (rng, k)
        finally:
            eng.close()
    # two engine shards give the rows of one engine over the whole range
    whole, a, b = g.Batched2048(512, seed=8), g.Batched2048(200, seed=8), g.Batched2048(312, seed=8, board_offset=200)
    try:
        for e in (whole, a, b):
            e.reset()
        torch.cuda.synchronize()
        assert np.array_equal(np.concatenate([a.get_boards(), b.get_boards()]), whole.get_boards())   # the spawn stream's own index rule
        w, x, y = (e.mc_search(16, 30, seed=3) for e in (whole, a, b))
        torch.cuda.synchronize()
        for k in range(3):
            assert torch.equal(torch.cat([x[k], y[k]]), w[k]), k
    finally:
        for e in (whole, a, b):
            e.close()


def test_after_a_graph_replay(g, torch_cuda):
    """A cached rollout graph is neither replayed nor invalidated by a search between two replays."""
    torch = torch_cuda
    n, k = 1024, 8
    eng, ref_eng = g.Batched2048(n, seed=11), g.Batched2048(n, seed=11)
    try:
        acts = torch.randint(0, 4, (k, n), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
        for e in (eng, ref_eng):
            e.reset()
        eng.rollout(acts)
        ref_eng.rollout(acts)
        before = eng.graph_replays
        eng.mc_search(8, 10, seed=1)
        assert eng.graph_replays == before
        eng.rollout(acts)
        ref_eng.rollout(acts)
        torch.cuda.synchronize()
        assert torch.equal(eng.records(), ref_eng.records()) and eng.clock == ref_eng.clock
        assert eng.graph_replays == ref_eng.graph_replays
    finally:
        eng.close()
        ref_eng.close()


@pytest.mark.parametrize("n", [1, 3, 63, 65, 4097])
def test_sentinel_tails_every_output_subset(g, torch_cuda, hm, n):
    """Each requested output is the head of a larger buffer filled with a sentinel: nothing past n is written, a field
    passed as None stays None, and what is written equals the host build.  Both lane groupings, both forms."""
    torch = torch_cuda
    boards = mixed_boards(n, 110 + n)
    dev = torch.as_tensor(boards).cuda()
    eng = g.Batched2048(n)
    try:
        eng.set_boards(boards)
        for R, L in ((5, 12), (35, 9)):
            host = host_mc(hm, boards, R, L)
            names = ("action", "value", "steps")
            for bits in range(1, 8):
                subset = [names[k] for k in range(3) if bits >> k & 1]
                for form in ("plain", "engine"):
                    bufs = {"action": torch.full((n + 4096,), 0xA5, dtype=torch.uint8, device="cuda"),
                            "value": torch.full((4 * n + 4096,), -0x5A5A5A5A5A5A, dtype=torch.int64, device="cuda"),
                            "steps": torch.full((4 * n + 4096,), -0x3C3C3C3C3C3C, dtype=torch.int64, device="cuda")}
                    sentinel = {k: v[-1].item() for k, v in bufs.items()}
                    out = g.MCSearch(*[(bufs[k][:n] if k == "action" else bufs[k][:4 * n].view(n, 4)) if k in subset else None
                                       for k in names])
                    res = g.mc_search(dev, R, L, SEED, out=out) if form == "plain" else eng.mc_search(R, L, seed=SEED, out=out)
                    torch.cuda.synchronize()
                    where = (R, subset, form)
                    for k, name in enumerate(names):
                        size = n if name == "action" else 4 * n
                        assert (getattr(res, name) is None) == (name not in subset), where
                        if name in subset:
                            assert np.array_equal(bufs[name][:size].cpu().numpy().reshape(host[k].shape), host[k]), where
                        assert bool((bufs[name][size if name in subset else 0:] == sentinel[name]).all()), where
    finally:
        eng.close()


def test_out_reuse_and_stream_order(g, torch_cuda):
    torch = torch_cuda
    n = 5000
    boards = torch.as_tensor(mixed_boards(n, 30)).cuda()
    want = g.mc_search(boards, 6, 20, seed=9)
    out = g.MCSearch(torch.full((n,), 7, dtype=torch.uint8, device="cuda"), torch.zeros((n, 4), dtype=torch.int64, device="cuda"),
                     torch.zeros((n, 4), dtype=torch.int64, device="cuda"))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        src = torch.empty_like(boards)
        torch.cuda._sleep(1 << 20)           # the copy below lands late: a search on another stream would see garbage
        src.copy_(boards)
        got = g.mc_search(src, 6, 20, seed=9, out=out)
    torch.cuda.synchronize()
    assert all(a is b for a, b in zip(got, out))
    for a, b in zip(out, want):
        assert torch.equal(a, b)
    # the same buffers again with other parameters: fully overwritten
    g.mc_search(boards, 40, 5, seed=10, out=out)
    fresh = g.mc_search(boards, 40, 5, seed=10)
    torch.cuda.synchronize()
    for a, b in zip(out, fresh):
        assert torch.equal(a, b)
    assert not torch.equal(fresh.value, want.value)


@pytest.mark.parametrize("R,G", [(4, 16), (32, 64)])
def test_grid_stride_passes(g, torch_cuda, hm, R, G):
    """n * G lanes past the grid cap: every board after the first pass is reached by the kernel's stride loop, the last
    pass ragged.  The board index is part of the Philox counter, so slices of the large batch (first, last, one across
    each pass boundary) are compared with plain calls on those slices at the matching index_offset, and with the host."""
    torch = torch_cuda
    assert (R >= WAVE_ROLLOUTS) == (G == 64)
    L, off = 6, 1 << 20
    stride = SEARCH_MAX_LANES // G                                   # boards per pass
    n = 2 * stride + 4133
    assert n > 2 * stride and n % stride != 0                        # three passes, the last ragged
    base = torch.as_tensor(mixed_boards(4099, 80)).cuda()
    boards = base.repeat(-(-n // len(base)), 1)[:n].contiguous()
    big = g.mc_search(boards, R, L, SEED, index_offset=off)
    torch.cuda.synchronize()
    for lo in (0, stride - 300, 2 * stride - 300, n - 600):
        hi = lo + 600
        part = g.mc_search(boards[lo:hi].contiguous(), R, L, SEED, index_offset=off + lo)
        torch.cuda.synchronize()
        for k in range(3):
            assert torch.equal(big[k][lo:hi], part[k]), (lo, k)
        assert_same(to_np(part), host_mc(hm, boards[lo:hi].cpu().numpy(), R, L, index_offset=off + lo), lo)
    # equal boards one period apart sit at different indices and give different values
    assert not torch.equal(big.value[:4099], big.value[4099:2 * 4099])
    eng = g.Batched2048(n, board_offset=off)
    try:
        eng.set_boards(boards)
        s = eng.mc_search(R, L, seed=SEED)
        torch.cuda.synchronize()
        for k in range(3):
            assert torch.equal(s[k], big[k]), k
    finally:
        eng.close()


def test_mc_plays_well(g, torch_cuda):
    """512 games to the end: never an illegal move while a legal one exists, and a mean final score of at least 10 x the
    random policy's (the bar of test_depth1_plays_well).  On the CPU the definition itself (host build, R = 16, 24 games)
    scores a mean of 16 402 against the random policy's 47.5 (tests/test_mc_host.py); on the MI355X this test measured
    30 550 against 66.4 (profiles/r09_mc_probe.txt)."""
    from gym2048_amd.transitions import mc_step_seed
    n, seed = 512, 2048   # the Monte-Carlo player: R = 64, playouts to the end, a seed per step
    searched, illegal, *_ = play(g, torch_cuda, n, seed, lambda eng, t: eng.mc_search(64, seed=mc_step_seed(seed, t)).action)
    rand, *_ = play(g, torch_cuda, n, seed, random_policy(torch_cuda, n, seed))
    print(f"mc R=64 mean final score {searched.mean():.1f}, random {rand.mean():.1f}")
    assert not illegal, "the search picked an illegal move while a legal one existed"
    assert (searched >= 0).all() and (rand >= 0).all(), "a game outlived the 5 000-move cap"
    assert searched.mean() >= 10 * rand.mean(), (searched.mean(), rand.mean())


def test_record_search_mc(g, torch_cuda):
    from gym2048_amd.batched import values_to_exp
    from gym2048_amd.transitions import Transitions, mc_step_seed
    torch = torch_cuda
    n, k, off = 64, 12, 500
    eng = g.Batched2048(n, seed=9, board_offset=off)
    try:
        eng.reset()
        clock0 = eng.clock
        tr = Transitions.record_search(eng, k, player="mc", rollouts=8, max_steps=40, seed=77)
        assert eng.clock == clock0 + k
    finally:
        eng.close()
    assert tr.size() == n * k
    boards = values_to_exp(tr.x).reshape(n, k, 16).astype(np.uint8)
    acts = tr.action.reshape(n, k)
    for j in range(k):   # step j searched its boards under the seed of clock0 + j
        s = g.mc_search(torch.as_tensor(np.ascontiguousarray(boards[:, j])).cuda(), 8, 40, mc_step_seed(77, clock0 + j), index_offset=off)
        assert np.array_equal(acts[:, j], s.action.cpu().numpy()), j
    assert len({mc_step_seed(77, clock0 + j) for j in range(k)}) == k
