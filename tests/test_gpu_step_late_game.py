"""GPU: every launch form that advances a game -- step_kernel's 32 instantiations, step_graph_kernel, rollout_random_kernel,
rollout_fused_kernel, step_numpy_kernel, rollout_fused_numpy_kernel, the two-chain split, step_host -- started from the
engineered late-game boards of tests/late_game.py instead of reset(): the spawn into the last empty cell and the end test
behind it, full boards, terminal boards, max_tile, the deficit carry across the record's registers, 2^16 / 2^17 merges.
Every expected value is the C oracle's; every comparison is exact.  tests/test_late_game_host.py proves on the CPU that
the families reach those states."""
import functools
import itertools

import numpy as np
import pytest

import late_game as lg
from oracle.cpu_ref import random_actions_np

pytestmark = pytest.mark.gpu
K = 11                                                       # fused: one double group of eight steps and a three-step tail
OBS_DTYPES = ("uint8", "float16", "float32")


@functools.lru_cache(maxsize=None)
def batches():
    """name -> family-shaped batch: "mixed" (every family of the common configuration, a whole number of blocks), "ragged"
    (the same without its last three boards), the single families, and "chains" (every fifth board of mixed)."""
    mixed = lg.mixed_families()
    out = {f.name: f for f in mixed + lg.max_tile_families()}
    out["rows"] = lg.rows_family()
    out["mixed"], out["ragged"] = lg.concat(mixed), lg.concat(mixed, drop=3)
    for drop, fam in ((3, out["max_tile_2048"]), (3, out["max_tile_top"])):
        out[fam.name + "_ragged"] = lg.concat([fam], drop=drop)
    m, pick = out["mixed"], np.arange(4096) * 5
    out["chains"] = lg.Family("chains", m.boards[pick], m.scores[pick], m.actions[pick], lambda f, o: None, m.max_tile,
                              m.illegal_move_reward, m.clock, offset=7 << 20)
    assert m.n % 256 == 0 and out["ragged"].n % 256 != 0 and out["chains"].n == 4096
    return out


class Pair:
    """An engine and the oracle in the same engineered state; the oracle's steps are range-checked and its books kept."""

    def __init__(self, torch, fam, rng="philox", chains=None):
        from gym2048_amd.batched import Batched2048
        from oracle import OracleBatch
        self.torch, self.fam, self.numpy_mode = torch, fam, rng == "numpy"
        self.eng = Batched2048(fam.n, seed=lg.SEED, board_offset=fam.offset, illegal_move_reward=fam.illegal_move_reward,
                               max_tile=fam.max_tile, rng=rng, chains=chains)
        self.ora = OracleBatch(fam.n, lg.SEED, fam.offset, threads=0)
        if self.numpy_mode:
            self.ora.seed_numpy(lg.SEED)
        self.illegal_ends = 0
        self.install()

    def install(self):
        """The engineered state on both sides (again: between two runs over the same buffers)."""
        self.eng.set_boards(self.fam.boards)
        self.eng.set_scores(self.fam.scores)
        self.eng.set_clock(self.fam.clock)
        lg.install(self.ora, self.fam)

    def oracle_step(self, actions, auto_reset=True, first=False):
        o = self.ora
        (o.step_numpy if self.numpy_mode else o.step)(actions, auto_reset=auto_reset)
        lg.check_scores(o)
        if first and actions is not None and not self.numpy_mode:
            self.fam.check(o)                                # the family reached what it names
        self.illegal_ends += int(((o.illegal != 0) & (o.terminated != 0)).sum())
        return o

    def check_state(self, where=None):
        e, o = self.eng, self.ora
        assert np.array_equal(e.get_boards().reshape(-1, 16), o.boards), where
        assert np.array_equal(e.get_scores(), o.score), where
        assert np.array_equal(e.get_last_scores(), o.last_score), where
        assert e.clock == o.t, where
        if self.numpy_mode:
            assert np.array_equal(e.get_numpy_rng().T, o.rng), where
        raw = e.records().cpu().numpy()                      # the deficit in the spare bits of bytes 8..15, nothing in 0..7
        assert np.array_equal(raw & 0x1F, o.boards) and not (raw[:, :8] & 0xE0).any(), where
        assert np.array_equal(lg.record_deficit(raw), (lg.potential(o.boards) - o.score) % lg.SCORE_LIMIT), where

    def check_books(self, where=None):
        st, o = self.eng.episode_stats(), self.ora
        had = o.ep_count > 0
        assert st["episodes"] == int(o.ep_count.sum()) and st["illegal_ends"] == self.illegal_ends, where
        assert st["return_sum"] == o.return_sum, where
        assert st["last_score_max"] == (int(o.last_score[had].max()) if had.any() else 0), where
        assert st["max_exp"] == int(o.boards.max()), where

    def close(self):
        self.eng.close()


def check_outputs(o, reward, terminated, illegal=None, highest=None, terminal_boards=None, where=None):
    """One step's outputs (numpy) against the oracle's."""
    assert np.array_equal(reward, o.reward), ("reward", where)
    assert np.array_equal(terminated, o.terminated), ("terminated", where)
    if illegal is not None:
        assert np.array_equal(illegal, o.illegal), ("illegal", where)
    if highest is not None:
        assert np.array_equal(highest, o.highest), ("highest", where)
    if terminal_boards is not None:
        done = o.terminated != 0
        assert np.array_equal(terminal_boards.reshape(-1, 16)[done], o.terminal_boards[done]), ("terminal_boards", where)


def guarded_obs(torch, device, lead, n, dtype_name):
    """(flat, view): an observation buffer of lead x n boards with one guard board behind the last, filled with 9."""
    rows = int(np.prod(lead, dtype=np.int64)) * n
    flat = torch.full((rows + 1, 16, 4, 4), 9, dtype=getattr(torch, dtype_name), device=device)
    return flat, flat[:rows].view(*lead, n, 16, 4, 4)


def action_rows(pair, k, dtype_name):
    """[k, n] action tensor: row 0 the family's actions, the rest the engine's own synthetic policy for those steps."""
    torch, eng = pair.torch, pair.eng
    acts = eng.random_actions(k)
    acts[0] = torch.as_tensor(pair.fam.actions, device=eng.device)
    return acts.to(getattr(torch, dtype_name))


# ------------------------------------------------------------------------------------ 1. step(): all 32 step_kernel forms
SOURCES = (None, "uint8", "int32", "int64")
STEP_CASES = list(itertools.product(range(4), (False, True), (True, False), (False, True)))   # source, ragged, info, obs


def _obs_dtype(src, ragged, want_info):
    return OBS_DTYPES[(4 * src + 2 * ragged + (not want_info)) % 3]


# every observation dtype meets both want_info values and both batch shapes
for _dt in OBS_DTYPES:
    _met = {(r, i) for s, r, i, obs in STEP_CASES if obs and _obs_dtype(s, r, i) == _dt}
    assert {r for r, i in _met} == {False, True} and {i for r, i in _met} == {False, True}


def _step_form(torch, fam, src, want_info, with_obs, obs_dtype, auto_reset):
    pair = Pair(torch, fam)
    try:
        eng, n = pair.eng, fam.n
        flat = obs = None
        if with_obs:
            flat, obs = guarded_obs(torch, eng.device, (), n, obs_dtype)
        for s in range(3):                                   # one step from the engineered state, then two more
            if SOURCES[src] is None:
                a_np = a_dev = None
            else:
                a_np = fam.actions if s == 0 else random_actions_np(lg.SEED, fam.clock + 1 + s, fam.offset, n)
                a_dev = torch.as_tensor(a_np).to(getattr(torch, SOURCES[src]))
            r, t = eng.step(a_dev, auto_reset=auto_reset, want_info=want_info, obs=obs)
            o = pair.oracle_step(a_np, auto_reset, first=s == 0)
            info = (eng.illegal.cpu().numpy(), eng.highest.cpu().numpy(), eng.terminal_boards.cpu().numpy()) if want_info else ()
            check_outputs(o, r.cpu().numpy(), t.cpu().numpy(), *info, where=s)
            if with_obs:
                assert np.array_equal(obs.cpu().numpy(), o.onehot().astype(obs_dtype)), s
                assert bool((flat[n] == 9).all()), "the fused observation wrote past the last board"
            pair.check_state(s)
        pair.check_books()
    finally:
        pair.close()


@pytest.mark.parametrize("src,ragged,want_info,with_obs", STEP_CASES)
def test_step_every_instantiation(torch_cuda, src, ragged, want_info, with_obs):
    """step() over action source x whole / ragged blocks x want_info x fused observation = step_kernel<ACT, FULL, STD, OBS>,
    on the mixed batch (about 20 000 boards); the max-tile families in engines of their own (they run STD = false only)."""
    obs_dtype = _obs_dtype(src, ragged, want_info)
    auto_reset = (src + ragged + want_info + with_obs) % 2 == 0
    b = batches()
    for name in ("mixed", "max_tile_2048", "max_tile_top"):
        fam = b["ragged" if name == "mixed" else name + "_ragged"] if ragged else b[name]
        _step_form(torch_cuda, fam, src, want_info, with_obs, obs_dtype, auto_reset)


# --------------------------------------------------------------------------------------------------------------- 2. rows
@pytest.mark.parametrize("form", ["info", "obs", "fused"])
def test_rows_one_step(torch_cuda, form):
    """All 18^4 rows in four orientations, 104 976 boards, one step: through the move, the spawn and the end test."""
    torch = torch_cuda
    fam = batches()["rows"]
    pair = Pair(torch, fam)
    try:
        eng, n = pair.eng, fam.n
        acts = torch.as_tensor(fam.actions, device=eng.device)
        auto_reset = form != "obs"
        o = pair.oracle_step(fam.actions, auto_reset, first=True)
        if form == "info":
            r, t = eng.step(acts, auto_reset=auto_reset, want_info=True)
            check_outputs(o, r.cpu().numpy(), t.cpu().numpy(), eng.illegal.cpu().numpy(), eng.highest.cpu().numpy(),
                          eng.terminal_boards.cpu().numpy())
        elif form == "obs":
            flat, obs = guarded_obs(torch, eng.device, (), n, "uint8")
            r, t = eng.step(acts.to(torch.int32), auto_reset=auto_reset, want_info=False, obs=obs)
            check_outputs(o, r.cpu().numpy(), t.cpu().numpy())
            assert np.array_equal(obs.cpu().numpy(), o.onehot()) and bool((flat[n] == 9).all())
        else:
            out = {key: torch.full((1, n), 7, dtype=torch.float32 if key == "reward" else torch.uint8, device=eng.device)
                   for key in ("reward", "terminated", "illegal", "highest")}
            eng.rollout(acts.view(1, n), auto_reset=auto_reset, fused=True, **out)
            check_outputs(o, *(out[key][0].cpu().numpy() for key in ("reward", "terminated", "illegal", "highest")))
        pair.check_state()
        pair.check_books()
    finally:
        pair.close()


# ------------------------------------------------------------------------------------------- 3. / 4. rollout, [k, n] buffers
@pytest.mark.parametrize("auto_reset", [True, False])
def test_rollout_every_optional_output(torch_cuda, auto_reset):
    torch = torch_cuda
    fam = batches()["ragged"]
    pair = Pair(torch, fam)
    try:
        eng, n, dev = pair.eng, fam.n, pair.eng.device
        acts = action_rows(pair, K, "uint8")
        out = {key: torch.full((K, n), 7, dtype=torch.float32 if key == "reward" else torch.uint8, device=dev)
               for key in ("reward", "terminated", "illegal", "highest")}
        tb = torch.full((K, n, 16), 77, dtype=torch.uint8, device=dev)
        flat, obs = guarded_obs(torch, dev, (K,), n, "uint8")
        eng.rollout(acts, auto_reset=auto_reset, terminal_boards=tb, obs=obs, **out)
        got = {key: v.cpu().numpy() for key, v in out.items()}
        tb_np, obs_np = tb.cpu().numpy(), obs.cpu().numpy()
        for j in range(K):
            o = pair.oracle_step(fam.actions if j == 0 else None, auto_reset, first=j == 0)
            check_outputs(o, got["reward"][j], got["terminated"][j], got["illegal"][j], got["highest"][j], tb_np[j], where=j)
            assert (tb_np[j][o.terminated == 0] == 77).all(), j          # rows are written only where an episode ended
            assert np.array_equal(obs_np[j], o.onehot()), j
        assert bool((flat[K * n] == 9).all()), "the fused observation wrote past the last board"
        pair.check_state()
        pair.check_books()
    finally:
        pair.close()


@pytest.mark.parametrize("name", ["mixed", "ragged"])
def test_rollout_standard_outputs_twice_second_from_the_cached_graph(torch_cuda, name):
    """Reward and terminated only, twice over the same buffers from the same engineered state: the second run is a replay of
    the cached graph (step_graph_kernel<ACT, FULL>)."""
    torch = torch_cuda
    fam = batches()[name]
    pair = Pair(torch, fam)
    try:
        eng, n, dev = pair.eng, fam.n, pair.eng.device
        if eng.graph_status != "":
            pytest.skip(eng.graph_status)
        acts = action_rows(pair, K, "int64" if name == "mixed" else "uint8")
        rew = torch.zeros((K, n), dtype=torch.float32, device=dev)
        term = torch.zeros((K, n), dtype=torch.uint8, device=dev)
        for run in range(2):
            if run:
                pair.install()
                rew.fill_(7.0)
                term.fill_(7)
            replays = eng.graph_replays
            eng.rollout(acts, reward=rew, terminated=term)
            if eng.graph_status != "":
                pytest.skip(eng.graph_status)
            assert eng.graph_replays == replays + run
            got_r, got_t = rew.cpu().numpy(), term.cpu().numpy()
            for j in range(K):
                o = pair.oracle_step(fam.actions if j == 0 else None, first=j == 0)
                check_outputs(o, got_r[j], got_t[j], where=(run, j))
            pair.check_state(run)
            pair.check_books(run)
    finally:
        pair.close()


# ------------------------------------------------------------------------------------------------- 5. / 6. fused rollouts
@pytest.mark.parametrize("source", ["uint8", "int32", "int64", "k"])
def test_rollout_fused(torch_cuda, source):
    torch = torch_cuda
    fam = batches()["ragged" if source in ("int32", "k") else "mixed"]
    auto_reset = source != "int32"
    pair = Pair(torch, fam)
    try:
        eng, n = pair.eng, fam.n
        acts = K if source == "k" else action_rows(pair, K, source)
        out = {key: torch.full((K, n), 7, dtype=torch.float32 if key == "reward" else torch.uint8, device=eng.device)
               for key in ("reward", "terminated", "illegal", "highest")}
        eng.rollout(acts, auto_reset=auto_reset, fused=True, **out)
        got = {key: v.cpu().numpy() for key, v in out.items()}
        for j in range(K):
            o = pair.oracle_step(fam.actions if j == 0 and source != "k" else None, auto_reset, first=j == 0)
            check_outputs(o, got["reward"][j], got["terminated"][j], got["illegal"][j], got["highest"][j], where=j)
        pair.check_state()
        pair.check_books()
    finally:
        pair.close()


@pytest.mark.parametrize("name", ["mixed", "ragged", "max_tile_2048"])
def test_rollout_random(torch_cuda, name):
    pair = Pair(torch_cuda, batches()[name])
    try:
        pair.eng.rollout_random(K)
        for j in range(K):
            pair.oracle_step(None)
        pair.check_state()
        pair.check_books()
    finally:
        pair.close()


# ------------------------------------------------------------------------------------------------------------ 7. two chains
def test_two_chain_rollout(torch_cuda):
    """set_chains(2), 4 096 boards, 64 steps: long enough to be split while the side chain is cold."""
    torch = torch_cuda
    fam = batches()["chains"]
    k = 64
    pair = Pair(torch, fam, chains=2)
    try:
        eng, n, dev = pair.eng, fam.n, pair.eng.device
        acts = action_rows(pair, k, "uint8")
        rew = torch.zeros((k, n), dtype=torch.float32, device=dev)
        term = torch.zeros((k, n), dtype=torch.uint8, device=dev)
        eng.rollout(acts, reward=rew, terminated=term)
        assert eng.chains_used == 2
        got_r, got_t = rew.cpu().numpy(), term.cpu().numpy()
        for j in range(k):
            o = pair.oracle_step(fam.actions if j == 0 else None)
            check_outputs(o, got_r[j], got_t[j], where=j)
        pair.check_state()
        pair.check_books()
    finally:
        pair.close()


# --------------------------------------------------------------------------------------------------------- 8. numpy-RNG mode
@pytest.mark.parametrize("form", ["step", "fused"])
@pytest.mark.parametrize("name", ["one_hole", "full_a", "full_b", "carry"])
def test_numpy_rng_mode(torch_cuda, name, form):
    """step_numpy_kernel / rollout_fused_numpy_kernel.  With one empty cell the reference's position draw is a choice among
    one, after an illegal move it draws nothing: the generator states tell whether the device consumed what numpy does."""
    torch = torch_cuda
    fam = batches()[name]
    auto_reset = name != "full_b"
    pair = Pair(torch, fam, rng="numpy")
    try:
        eng, n = pair.eng, fam.n
        assert np.array_equal(eng.get_numpy_rng().T, pair.ora.rng)
        if form == "step":
            for s in range(3):
                a = fam.actions if s == 0 else random_actions_np(lg.SEED, fam.clock + 1 + s, fam.offset, n)
                r, t = eng.step(torch.as_tensor(a), auto_reset=auto_reset)
                o = pair.oracle_step(a, auto_reset)
                check_outputs(o, r.cpu().numpy(), t.cpu().numpy(), eng.illegal.cpu().numpy(), eng.highest.cpu().numpy(),
                              eng.terminal_boards.cpu().numpy(), where=s)
                pair.check_state(s)
        else:
            acts = action_rows(pair, K, "int32")
            out = {key: torch.full((K, n), 7, dtype=torch.float32 if key == "reward" else torch.uint8, device=eng.device)
                   for key in ("reward", "terminated", "illegal", "highest")}
            eng.rollout(acts, auto_reset=auto_reset, fused=True, **out)
            got = {key: v.cpu().numpy() for key, v in out.items()}
            for j in range(K):
                o = pair.oracle_step(fam.actions if j == 0 else None, auto_reset)
                check_outputs(o, got["reward"][j], got["terminated"][j], got["illegal"][j], got["highest"][j], where=j)
            pair.check_state()
        pair.check_books()
    finally:
        pair.close()


# --------------------------------------------------------------------------------------------------------------- 9. step_host
@pytest.mark.parametrize("name,auto_reset", [("one_hole", True), ("full_a", True), ("full_b", False)])
def test_step_host(torch_cuda, name, auto_reset):
    torch = torch_cuda
    fam = batches()[name]
    pair = Pair(torch, fam)
    try:
        eng, n = pair.eng, fam.n
        io = eng.host_io()
        for s in range(3):
            a = fam.actions if s == 0 else random_actions_np(lg.SEED, fam.clock + 1 + s, fam.offset, n)
            io["actions"][:] = a
            out = eng.step_host(auto_reset)
            o = pair.oracle_step(a, auto_reset, first=s == 0)
            check_outputs(o, out["reward"], out["terminated"], out["illegal"], out["highest"], out["terminal_boards"], where=s)
            assert np.array_equal(out["boards"].reshape(n, 16), o.boards), s
            pair.check_state(s)
        assert np.array_equal(eng.fetch_host()["scores"], pair.ora.score)
        pair.check_books()
    finally:
        pair.close()
