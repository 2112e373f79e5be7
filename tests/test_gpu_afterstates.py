"""GPU: afterstates (g2048_afterstates / g2048_afterstates_plain, Batched2048.afterstates, gym2048_amd.afterstates)
against the reference's move table, the exhaustive shift() table, an oracle row table at 2^20 live boards, the engine's
own move / legal_actions / step, and with no side effect on the engine."""
import itertools

import numpy as np
import pytest

from conftest import load_golden
from analysis_helpers import row_lut  # noqa: F401 (fixture)
from move_lut import lut_afterstates

DTYPES = ("uint8", "float16", "float32")


# ---------------------------------------------------------------------------------------------- numpy checkers
def stack_np(boards):
    """stack() (game2048_env.py:17-32) of [..., 16] exponents -> [..., 16, 4, 4] uint8; pinned to stack_table below."""
    b = np.asarray(boards)
    oh = (b[..., None, :] == np.arange(16, dtype=b.dtype)[:, None]).astype(np.uint8)
    return oh.reshape(b.shape[:-1] + (16, 4, 4))


def test_numpy_checkers_pinned(row_lut):
    s = load_golden("stack_table")
    assert np.array_equal(stack_np(s["boards"]), s["onehot"])
    m = load_golden("move_table")
    if m["boards"].max() < 18:
        new, score, mask = lut_afterstates(m["boards"], row_lut)
        assert np.array_equal(new, m["new"]) and np.array_equal(score, np.where(m["legal"], m["score"], 0))


def both_forms(torch, boards, obs_dtype=None):
    """(engine form, plain form) of the same [n,16] boards."""
    from gym2048_amd.batched import Batched2048, afterstates
    n = len(boards)
    eng = Batched2048(n)
    eng.set_boards(boards)
    a = eng.afterstates(obs_dtype=obs_dtype)
    dev = torch.as_tensor(np.ascontiguousarray(boards, dtype=np.uint8).reshape(n, 16)).to("cuda:0")
    b = afterstates(dev, obs_dtype=obs_dtype)
    torch.cuda.synchronize()
    eng.close()
    return a, b


# ---------------------------------------------------------------------------------------------- 1. move table
@pytest.mark.gpu
def test_move_table_both_forms(torch_cuda):
    torch = torch_cuda
    m = load_golden("move_table")
    want_mask = (m["legal"].astype(np.uint8) << np.arange(4, dtype=np.uint8)).sum(axis=1).astype(np.uint8)
    want_obs = stack_np(m["new"])
    for dt in DTYPES:
        for res in both_forms(torch, m["boards"], getattr(torch, dt)):
            assert np.array_equal(res.boards.cpu().numpy(), m["new"])
            assert np.array_equal(res.score.cpu().numpy(), np.where(m["legal"], m["score"], 0))
            assert np.array_equal(res.legal.cpu().numpy(), want_mask)
            assert res.obs.dtype == getattr(torch, dt) and tuple(res.obs.shape) == (len(m["boards"]), 4, 16, 4, 4)
            assert np.array_equal(res.obs.to(torch.uint8).cpu().numpy(), want_obs)


# ---------------------------------------------------------------------------------------------- 2. shift() exhaustive
@pytest.mark.gpu
def test_shift_exhaustive_all_directions_both_forms(torch_cuda):
    """All 104 976 rows of shift() (exponents 0..17), four rows per board, in each direction with the transposes of
    test_gpu_parity.test_shift_exhaustive."""
    torch = torch_cuda
    g = load_golden("shift_exhaustive")
    rows = np.array(np.meshgrid(*[np.arange(18)] * 4, indexing="ij")).reshape(4, -1).T.astype(np.uint8)
    n = len(rows) // 4
    b = rows.reshape(n, 4, 4)
    t = lambda x: x.transpose(0, 2, 1)            # noqa: E731
    want_score = g["score"].reshape(n, 4).sum(axis=1)
    cases = {  # direction: (board fed in, afterstate -> rows in left-move order)
        3: (b, lambda y: y),
        0: (t(b), t),
        1: (b[:, :, ::-1], lambda y: y[:, :, ::-1]),
        2: (t(b)[:, ::-1, :], lambda y: t(y[:, ::-1, :])),
    }
    for d, (fed, back) in cases.items():
        fed = np.ascontiguousarray(fed).reshape(n, 16)
        for res in both_forms(torch, fed):
            after = res.boards.cpu().numpy()[:, d].reshape(n, 4, 4)
            assert np.array_equal(back(after).reshape(-1, 4), g["out"]), d
            assert np.array_equal(res.score.cpu().numpy()[:, d], want_score), d
            legal = (res.legal.cpu().numpy() >> d) & 1
            assert np.array_equal(legal.astype(bool), (after.reshape(n, 16) != fed).any(axis=1)), d


# ---------------------------------------------------------------------------------------------- 3. live boards at 2^20
@pytest.mark.gpu
def test_live_boards_2p20_against_row_table_and_engine(torch_cuda, row_lut):
    torch = torch_cuda
    import torch.nn.functional as F
    from gym2048_amd.batched import Batched2048, afterstates
    n = 1 << 20
    eng = Batched2048(n, seed=2024)
    eng.reset(seed=2024)
    eng.rollout_random(96)
    boards = eng.boards().view(n, 16)
    a = eng.afterstates(obs_dtype=torch.uint8)
    p = afterstates(boards, obs_dtype=torch.uint8)
    torch.cuda.synchronize()
    for name in ("boards", "score", "legal", "obs"):
        assert torch.equal(getattr(a, name), getattr(p, name)), name
    new, score, mask = lut_afterstates(boards.cpu().numpy(), row_lut)
    assert np.array_equal(a.boards.cpu().numpy(), new)
    assert np.array_equal(a.score.cpu().numpy(), score)
    assert np.array_equal(a.legal.cpu().numpy(), mask)
    assert torch.equal(a.legal, eng.legal_actions())
    for d in range(4):
        s, legal = eng.move(torch.full((n,), d, dtype=torch.int64, device="cuda:0"), trial=True)
        assert torch.equal(a.score[:, d], s), d
        assert torch.equal(((a.legal >> d) & 1), legal), d
    chunk = 1 << 16
    for k in range(0, n, chunk):   # F.one_hot in int64: chunked
        want = F.one_hot(a.boards[k:k + chunk].long(), 16).permute(0, 1, 3, 2).reshape(-1, 4, 16, 4, 4).to(torch.uint8)
        assert torch.equal(a.obs[k:k + chunk], want)
    sub = boards[: 1 << 18]
    for dt in (torch.float16, torch.float32):
        q = afterstates(sub, obs_dtype=dt)
        want = F.one_hot(q.boards.long(), 16).permute(0, 1, 3, 2).reshape(-1, 4, 16, 4, 4).to(dt)
        assert torch.equal(q.obs, want), dt
        assert torch.equal(q.boards, a.boards[: 1 << 18])
    eng.close()


# ---------------------------------------------------------------------------------------------- 4. no side effects
@pytest.mark.gpu
@pytest.mark.parametrize("rng", ["philox", "numpy"])
def test_no_side_effects(torch_cuda, rng):
    torch = torch_cuda
    from gym2048_amd.batched import Batched2048
    n, seed = 4096 + 17, 99
    eng, twin = Batched2048(n, seed=seed, rng=rng), Batched2048(n, seed=seed, rng=rng)
    gen = torch.Generator(device="cpu").manual_seed(5)
    for e in (eng, twin):
        e.reset(seed=seed)
    for _ in range(40):
        acts = torch.randint(0, 4, (n,), generator=gen).to("cuda:0")
        eng.step(acts)
        twin.step(acts)
    torch.cuda.synchronize()
    rec, clock, stats = eng.records().clone(), eng.clock, eng.episode_stats()
    planes = eng.get_numpy_rng() if rng == "numpy" else None
    for dt in (None, torch.uint8, torch.float32):
        eng.afterstates(obs_dtype=dt)
    torch.cuda.synchronize()
    assert torch.equal(eng.records(), rec)
    assert eng.clock == clock
    assert eng.episode_stats() == stats
    if rng == "numpy":
        assert np.array_equal(eng.get_numpy_rng(), planes)
    for _ in range(40):
        acts = torch.randint(0, 4, (n,), generator=gen).to("cuda:0")
        ra, ta = (x.clone() for x in eng.step(acts))
        rb, tb = twin.step(acts)
        assert torch.equal(ra, rb) and torch.equal(ta, tb)
    assert torch.equal(eng.records(), twin.records())
    assert eng.episode_stats() == twin.episode_stats()
    eng.close()
    twin.close()


# ---------------------------------------------------------------------------------------------- 5. agreement with step
@pytest.mark.gpu
def test_step_is_afterstate_plus_one_spawn(torch_cuda):
    torch = torch_cuda
    from gym2048_amd.batched import Batched2048
    n = 1 << 16
    eng = Batched2048(n, seed=3)
    eng.reset(seed=3)
    eng.rollout_random(30)
    gen = torch.Generator(device="cpu").manual_seed(11)
    checked = 0
    for _ in range(8):
        a = eng.afterstates()
        acts = torch.randint(0, 4, (n,), generator=gen).to("cuda:0")
        chosen = a.boards[torch.arange(n, device="cuda:0"), acts]              # [n, 16]
        legal = ((a.legal >> acts.to(torch.uint8)) & 1).bool()
        want_reward = a.score.gather(1, acts.view(n, 1)).view(n)
        reward, _ = eng.step(acts, auto_reset=False)
        new = eng.boards().view(n, 16)
        diff = new != chosen
        assert torch.equal(diff.sum(1)[legal], torch.ones(int(legal.sum()), dtype=torch.int64, device="cuda:0"))
        cell = diff.float().argmax(1)
        rows = torch.arange(n, device="cuda:0")
        assert bool((chosen[rows, cell][legal] == 0).all())
        spawned = new[rows, cell][legal]
        assert bool(((spawned == 1) | (spawned == 2)).all())
        assert torch.equal(reward[legal], want_reward[legal].float())
        checked += int(legal.sum())
    assert checked > n
    eng.close()


# ---------------------------------------------------------------------------------------------- 6. ragged sizes, subsets
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 65, 1_000_003])
def test_ragged_sizes_every_output_subset(torch_cuda, n):
    torch = torch_cuda
    from gym2048_amd.batched import Afterstates, Batched2048, afterstates
    gen = torch.Generator(device="cpu").manual_seed(n)
    boards = torch.randint(0, 12, (n, 16), generator=gen, dtype=torch.uint8)
    boards[torch.rand((n, 16), generator=gen) < 0.4] = 0
    boards = boards.to("cuda:0")
    eng = Batched2048(n)
    eng.set_boards(boards)
    obs_dt = (torch.uint8, torch.float16, torch.float32, torch.uint8)[[1, 63, 65, 1_000_003].index(n)]
    full = afterstates(boards, obs_dtype=obs_dt)
    assert torch.equal(eng.afterstates(obs_dtype=obs_dt).boards, full.boards)
    shapes = {"boards": ((n, 4, 16), torch.uint8), "score": ((n, 4), torch.int32), "legal": ((n,), torch.uint8),
              "obs": ((n, 4, 16, 4, 4), obs_dt)}
    names = list(shapes)
    for k in range(1, 5):
        for subset in itertools.combinations(names, k):
            for form in ("engine", "plain"):
                # each requested output is the head of a larger buffer filled with a sentinel: nothing past n is written
                bufs, views = {}, {}
                for name in subset:
                    shape, dt = shapes[name]
                    per = int(np.prod(shape[1:], dtype=np.int64))
                    bufs[name] = torch.full((n * per + 4096,), 0x5A, dtype=dt, device="cuda:0")
                    views[name] = bufs[name][: n * per].view(shape)
                out = Afterstates(*(views.get(name) for name in names))
                res = eng.afterstates(out=out) if form == "engine" else afterstates(boards, out=out)
                torch.cuda.synchronize()
                for name in names:
                    if name in subset:
                        assert getattr(res, name) is views[name]
                        assert torch.equal(views[name], getattr(full, name)), (form, subset, name)
                        tail = bufs[name][n * int(np.prod(shapes[name][0][1:], dtype=np.int64)):]
                        assert bool((tail == 0x5A).all()), (form, subset, name)
                    else:
                        assert getattr(res, name) is None
    eng.close()
