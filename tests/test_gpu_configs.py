"""GPU: every BASELINE.json configuration at its REAL size against the oracle, through the C ABI.

  configs[1]  65 536 boards, random policy          -> tests/test_gpu_parity.py::test_random_rollout_vs_oracle
  configs[2]  2^20 boards, random policy            -> test_full_batch_2p20_random_policy_vs_oracle (full batch)
              + exactly as bench.py times it         -> test_bench_configuration_2p20_rollout_buffers_without_terminal_records
              + a legality-aware greedy policy (deep states: big tiles, full-board endings)
  configs[3]  shards of one batch on several ranks  -> test_two_rank_hip_shards_allgather (2 processes, gloo, cuda:0)
              + the N > 1 code path of bench.py over RCCL -> test_bench_forced_dist_runs_the_rccl_path (one-rank group)
  configs[4]  2^20 boards driving a torch policy    -> test_policy_loop_2p20_zero_copy_vs_oracle
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compare_state(eng, ora, step, fields=("boards", "score")):
    if "boards" in fields:
        assert np.array_equal(eng.get_boards().reshape(eng.n_envs, 16), ora.boards), f"boards differ at step {step}"
    if "score" in fields:
        assert np.array_equal(eng.get_scores(), ora.score), f"scores differ at step {step}"


def test_full_batch_2p20_random_policy_vs_oracle(torch_cuda):
    """BASELINE configs[2] at its real size: 2^20 boards x 40 steps of the synthetic random policy, the WHOLE
    batch bit for bit against the C oracle (all host cores) -- boards, scores, rewards, flags, every step."""
    from gym2048_amd.batched import Batched2048
    from oracle import OracleBatch
    n, seed, steps = 1 << 20, 42, 40
    eng, ora = Batched2048(n, seed=seed), OracleBatch(n, seed, threads=0)
    eng.reset()
    ora.reset()
    _compare_state(eng, ora, -1)
    for s in range(steps):
        eng.step(None)
        ora.step(None)
        assert np.array_equal(eng.reward.cpu().numpy(), ora.reward), s
        assert np.array_equal(eng.terminated.cpu().numpy(), ora.terminated), s
        assert np.array_equal(eng.illegal.cpu().numpy(), ora.illegal), s
        assert np.array_equal(eng.highest.cpu().numpy(), ora.highest), s
        _compare_state(eng, ora, s)
    assert np.array_equal(eng.get_last_scores(), ora.last_score)
    st = eng.episode_stats()
    assert st["episodes"] == int(ora.ep_count.sum()) > n


@pytest.mark.parametrize("chains", [1, 2])
def test_bench_configuration_2p20_rollout_buffers_without_terminal_records(torch_cuda, monkeypatch, chains):
    """The configuration bench.py times, at its real size and in BOTH launch forms it can take: 2^20 boards, the STANDARD
    step kernel through g2048_rollout over [K][B] uint8 action / float32 reward / uint8 terminated buffers, per-board
    terminal records OFF (g2048_set_last_records(0)); as one chain (one whole-batch launch per step: what the driver's
    K = 20 line runs) and as TWO chains (two half-batch launches per step on two streams: bench.py's default from K = 200;
    forced here for a 24-step rollout on a cold side chain by G2048_TWO_CHAIN_MIN_STEPS, which g2048_set_chains reads) --
    `chains_used` says which form really ran.  Every step's rewards and flags, the final boards and scores, the episode
    counters and the exact return sum against the C oracle; the calls that need terminal records refuse; switching them
    on again starts from "none yet" and from then on records exactly the episodes that end."""
    torch = torch_cuda
    from gym2048_amd._lib import G2048Error
    from gym2048_amd.batched import Batched2048, parse_stats
    from oracle import OracleBatch
    n, seed, k = 1 << 20, 42, 24
    if chains == 2:
        monkeypatch.setenv("G2048_TWO_CHAIN_MIN_STEPS", "2")
    eng, ora = Batched2048(n, seed=seed, last_records=False, chains=chains), OracleBatch(n, seed, threads=0)
    assert not eng.last_records_enabled and eng.chains == chains
    eng.reset()
    ora.reset()
    acts = eng.random_actions(k)
    rew = torch.zeros((k, n), dtype=torch.float32, device=eng.device)
    term = torch.zeros((k, n), dtype=torch.uint8, device=eng.device)
    eng.prepare_rollout(acts, reward=rew, terminated=term).run()
    assert eng.chains_used == chains, "the rollout did not run in the launch form this case is about"
    torch.cuda.synchronize()
    for j in range(k):
        ora.step(None)                                       # the synthetic policy = the generated actions
        assert np.array_equal(rew[j].cpu().numpy(), ora.reward), j
        assert np.array_equal(term[j].cpu().numpy(), ora.terminated), j
    _compare_state(eng, ora, k)
    st = eng.episode_stats()
    assert st["episodes"] == int(ora.ep_count.sum()) > n // 2
    assert st["return_sum"] == ora.return_sum == ora.finished_return_sum > 0
    assert st["last_count"] is st["last_score_sum"] is st["last_score_max"] is st["mean_last_score"] is None   # not kept: unknown, not 0
    ro = parse_stats(eng.episode_stats_device(returns_only=True))
    assert ro["last_count"] is None and ro["mean_last_score"] is None
    assert (ro["episodes"], ro["illegal_ends"], ro["return_sum"]) == (st["episodes"], st["illegal_ends"], st["return_sum"])
    for call in (eng.get_last_scores, eng.last_scores, eng.last_records):
        with pytest.raises(G2048Error, match="terminal records"):
            call()
    eng.set_last_records(True)
    assert eng.last_records_enabled and not eng.get_last_scores().any()
    ended = np.zeros(n, bool)
    for _ in range(6):
        eng.step(None)
        ora.step(None)
        ended |= ora.terminated.astype(bool)
    got = eng.get_last_scores()
    assert np.array_equal(got[ended], ora.last_score[ended]) and not got[~ended].any()
    _compare_state(eng, ora, k + 6)
    assert eng.episode_stats()["return_sum"] == ora.return_sum


def _greedy_actions(torch, eng):
    """Legality-aware greedy policy, computed on the device with trial moves (game2048_env.py:194-241,
    trial=True): the legal direction with the largest merge score, lowest direction on ties; 0 if none."""
    n = eng.n_envs
    best = torch.full((n,), -1, dtype=torch.int32, device=eng.device)
    choice = torch.zeros(n, dtype=torch.uint8, device=eng.device)
    for d in range(4):
        score, legal = eng.move(torch.full((n,), d, dtype=torch.uint8, device=eng.device), trial=True)
        val = torch.where(legal.bool(), score, torch.full_like(score, -1))
        better = val > best
        choice = torch.where(better, torch.full_like(choice, d), choice)
        best = torch.where(better, val, best)
    return choice


def test_full_batch_2p20_greedy_policy_vs_oracle(torch_cuda):
    """2^20 boards x 256 steps of a legality-aware greedy policy: no illegal moves, so episodes run until the
    board is full and stuck (game2048_env.py:262-280) and tiles grow to 2^8 and beyond -- spawn on nearly
    full boards, isend at depth, reset slot selection after a LEGAL move, scores in the thousands.  Whole
    batch against the oracle: rewards and flags every step, boards and scores every 16 steps."""
    torch = torch_cuda
    from gym2048_amd.batched import Batched2048
    from oracle import OracleBatch
    n, seed, steps = 1 << 20, 7, 256
    eng, ora = Batched2048(n, seed=seed, illegal_move_reward=-1.0), OracleBatch(n, seed, threads=0)
    ora.illegal_move_reward = -1.0
    eng.reset()
    ora.reset()
    natural_ends = 0
    for s in range(steps):
        acts = _greedy_actions(torch, eng)
        eng.step(acts)
        ora.step(acts.cpu().numpy())
        assert np.array_equal(eng.reward.cpu().numpy(), ora.reward), s
        assert np.array_equal(eng.terminated.cpu().numpy(), ora.terminated), s
        assert not ora.illegal.any(), "a legality-aware policy never makes an illegal move"
        natural_ends += int(ora.terminated.sum())
        if s % 16 == 15 or s == steps - 1:
            _compare_state(eng, ora, s)
            assert np.array_equal(eng.highest.cpu().numpy(), ora.highest), s
    assert np.array_equal(eng.get_last_scores(), ora.last_score)
    st = eng.episode_stats()
    assert st["episodes"] == natural_ends == int(ora.ep_count.sum()) and st["illegal_ends"] == 0
    assert natural_ends > n // 4, "hundreds of thousands of whole games played to a full, stuck board"
    assert st["max_exp"] >= 8 and st["last_score_max"] >= 2000, (st["max_exp"], st["last_score_max"])


def test_policy_loop_2p20_zero_copy_vs_oracle(torch_cuda):
    """BASELINE configs[4]: 2^20 boards driving a torch policy on the same GPU with zero host copies --
    g2048_onehot writes the (N,16,4,4) float16 observation INTO a caller-owned torch tensor, a small conv
    net (the shape of ppo_train.py:36-62: conv3x3 16->C, ReLU, flatten, linear -> 4 logits) picks argmax
    actions (int64), g2048_step reads that tensor's memory.  The int64 actions are copied out afterwards and
    the whole batch is replayed on the oracle."""
    torch = torch_cuda
    from gym2048_amd.batched import Batched2048
    from oracle import OracleBatch
    n, seed, steps = 1 << 20, 11, 12
    eng, ora = Batched2048(n, seed=seed), OracleBatch(n, seed, threads=0)
    eng.reset()
    ora.reset()
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")      # no exhaustive kernel search for a test
    torch.manual_seed(0)
    dev = eng.device
    conv = torch.nn.Conv2d(16, 8, 3, padding=1).to(dev).half()
    head = torch.nn.Linear(8 * 16, 4).to(dev).half()
    obs = torch.empty((n, 16, 4, 4), dtype=torch.float16, device=dev)
    actions = torch.empty(n, dtype=torch.int64, device=dev)    # what argmax produces; reused every step
    obs_ptr, act_ptr = obs.data_ptr(), actions.data_ptr()
    all_actions = torch.empty((steps, n), dtype=torch.int64, device=dev)
    chunk = 1 << 17                                            # the policy's forward batch (as bench_policy.py)
    with torch.no_grad():
        for s in range(steps):
            out = eng.observe_onehot(out=obs)
            assert out is obs and obs.data_ptr() == obs_ptr            # written in place, no new buffer
            for lo in range(0, n, chunk):
                logits = head(torch.relu(conv(obs[lo:lo + chunk])).flatten(1))
                actions[lo:lo + chunk] = logits.argmax(dim=1)            # int64, on the device
            assert actions.data_ptr() == act_ptr and eng._as_device(actions) is actions   # step() gets THIS memory
            eng.step(actions)
            all_actions[s] = actions
    torch.cuda.synchronize()
    # the observation the policy saw last is the one-hot of the boards before the last step: check a strided
    # sample of it against the oracle's stack() after replaying steps - 1 steps
    host_actions = all_actions.cpu().numpy()
    assert len(np.unique(host_actions)) > 1, "the policy should not be constant"
    for s in range(steps):
        if s == steps - 1:
            sample = np.arange(0, n, 4099)
            want = ora.onehot()[sample]
            assert np.array_equal(obs[torch.as_tensor(sample, device=dev)].cpu().numpy(), want.astype(np.float16))
        ora.step((host_actions[s] & 3).astype(np.uint8))
    _compare_state(eng, ora, steps)
    assert np.array_equal(eng.reward.cpu().numpy(), ora.reward)
    assert np.array_equal(eng.terminated.cpu().numpy(), ora.terminated)
    assert np.array_equal(eng.get_last_scores(), ora.last_score)


def test_two_rank_hip_shards_allgather(torch_cuda, tmp_path):
    """BASELINE configs[3]'s code path on one GPU: two processes (torch.distributed over gloo, both on
    cuda:0), each a HIP Batched2048 shard with its board_offset; the all-gathered episodic returns and
    the concatenated shard boards equal a single engine holding the whole batch."""
    from gym2048_amd.batched import Batched2048
    n, seed, k = 1 << 17, 42, 48
    port = 29500 + os.getpid() % 2000
    out = tmp_path / "gathered.npz"
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="2",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dist_hip_worker.py"), str(n), str(seed), str(k),
                               str(out)], env=dict(env, RANK=str(r)), cwd=ROOT) for r in range(2)]
    for p in procs:
        assert p.wait(timeout=600) == 0
    whole = Batched2048(n, seed=seed)
    whole.reset()
    whole.rollout(k)
    got = np.load(out)
    assert np.array_equal(got["returns"], whole.get_last_scores())
    assert np.array_equal(got["boards"], whole.get_boards().reshape(n, 16))
    st = whole.episode_stats()
    assert int(got["episodes"]) == st["episodes"] and int(got["last_sum"]) == st["last_score_sum"]
    assert int(got["last_max"]) == st["last_score_max"] and got["hist"].tolist() == st["highest_hist"]
    from gym2048_amd.batched import parse_stats
    want = {k: v for k, v in st.items() if k != "mean_episode_return"}      # (that one needs the engine's illegal_move_reward)
    assert parse_stats(whole.episode_stats_device()) == want                # async device struct == sync host struct
    ro = parse_stats(whole.episode_stats_device(returns_only=True))         # returns-only flavour: counts + exact return sum
    for key in ("episodes", "illegal_ends", "return_sum", "mean_episode_score"):
        assert ro[key] == st[key], key
    assert ro["max_exp"] == 0 and not any(ro["highest_hist"]) and ro["last_count"] is ro["last_score_sum"] is None
    assert int(got["return_sum"]) == st["return_sum"] > 0                   # the two shards' summaries add up to the whole


def _run_bench(argv, env):
    """bench.py as a subprocess.  A process-group rendezvous can fail for reasons that are not the code's (a port still
    in TIME_WAIT, a slow first RCCL initialisation on a fresh box): one retry on a fresh port, the first failure printed."""
    for attempt in (0, 1):
        if attempt and "MASTER_PORT" in env:
            env = dict(env, MASTER_PORT=str(int(env["MASTER_PORT"]) + 97))
        res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, env=env, cwd=ROOT, capture_output=True,
                             text=True, timeout=900)
        if res.returncode == 0:
            return res
        print(f"bench.py {argv} attempt {attempt} failed with {res.returncode}:\n{res.stderr[-3000:]}")
    assert res.returncode == 0, res.stderr[-3000:]


@pytest.mark.parametrize("gather", ["summary", "full"])
def test_bench_forced_dist_runs_the_rccl_path(torch_cuda, gather):
    """bench.py's N > 1 code path over the REAL backend on the one GPU there is: G2048_BENCH_FORCE_DIST=1 makes a
    one-rank `nccl` (= RCCL) process group, so init_process_group("nccl", device_id=...), the all-gather of a
    device tensor enqueued behind the K launches, the NCCL barrier and the max-reduction all execute.  The line
    must carry the timing split the scaling analysis needs, and the fixed cost the collective adds to the driver's
    20-launch train must stay small (DESIGN.md section 6 derives the predicted 8-GPU efficiency from it)."""
    import json
    env = dict(os.environ, G2048_BENCH_FORCE_DIST="1", MASTER_ADDR="127.0.0.1",
               MASTER_PORT=str(31000 + 2 * (os.getpid() % 1000) + (gather == "full")), HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    res = _run_bench(["--steps", "20", "--warmup", "5", "--no-extras", "--gather", gather], env)
    lines = res.stdout.strip().splitlines()
    assert lines[-1].startswith("{"), f"the JSON line must be the last line of stdout, got: {lines[-3:]}"
    line = json.loads(lines[-1])
    assert line["n_gpus"] == 1 and line["steps"] == 20 and "forced_dist" in line["config"]
    assert line["value"] > 1e10 and line["episodes_finished"] > 0
    # the line says what the process group really was, and runs in the same launch form as the N = 1 line at this K
    cfg = line["config"]
    assert cfg["backend"] == "nccl" and cfg["pg_world_size"] == 1 and cfg["gathered_rows"] == 1 and cfg["chains"] == 1
    assert len(line["timing"]["k_region_repeats_us"]) == 5 and 0 < line["roofline"]["frac_wall"] <= line["roofline"]["frac"]
    t = line["timing"]
    assert t["launch_train_us"] > 0 and t["collective_us"] > 0
    print(f"forced-dist ({gather}): launch train {t['launch_train_us']:.1f} us, collective {t['collective_us']:.1f} us, "
          f"host tail {t['host_tail_us']:.1f} us, value {line['value']:.3e}")
    # the regression bound over the SIX regions of the run, each exchange against ITS OWN launch train: one host hiccup on
    # a shared box (a 533 us exchange was seen once, the host reached it late) is not a failure, two are -- the
    # second-largest ratio must stay below a quarter (measured: 11-12 us behind a 195-200 us train for the summary,
    # ~20 us for --gather full; profiles/r06_*forced_dist*.txt)
    regions = sorted(zip([t["collective_us"]] + t["k_region_repeats_collective_us"],
                         [t["launch_train_us"]] + t["k_region_repeats_launch_train_us"]), key=lambda r: r[0] / r[1])
    assert len(regions) == 6 and regions[-2][0] < 0.25 * regions[-2][1], regions
    if gather == "summary":
        # one summary launch + one in-place ncclAllGather on the launch stream (round 5: a kernel pair + the process
        # group's all-gather with its stream hops, 26 us): the MEDIAN region stays within 14 us
        assert cfg["collective_path"].startswith("g2048_allgather_summary"), cfg
        assert sorted(r[0] for r in regions)[3] <= 14.0, regions
        assert line["global_returns"]["episodes"] == line["episodes_finished"]
        assert line["global_returns"]["return_sum"] == line["return_sum"] > 0
        assert line["global_returns"]["mean_episode_score"] == line["mean_episode_score"]


@pytest.mark.parametrize("gather", ["summary", "full"])
def test_bench_gpus_2_launches_itself(torch_cuda, gather):
    """The command the driver's scaling run uses -- plain `python bench.py --gpus N --steps 20 --warmup 5`, NO
    torch.distributed.run around it -- rehearsed with N = 2 on the one GPU there is: bench.py starts the two ranks
    itself (G2048_BENCH_SAME_DEVICE=1 puts both on cuda:0, G2048_BENCH_BACKEND=gloo carries the collectives, because
    RCCL refuses two ranks on one device), each rank steps its own HIP shard, the once-per-rollout exchange runs, and
    rank 0's JSON line comes back as the LAST line of the parent's stdout."""
    import json
    env = dict(os.environ, G2048_BENCH_BACKEND="gloo", G2048_BENCH_SAME_DEVICE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "G2048_BENCH_FORCE_DIST"):
        env.pop(k, None)
    res = _run_bench(["--gpus", "2", "--steps", "20", "--warmup", "5", "--no-extras", "--gather", gather], env)
    lines = res.stdout.strip().splitlines()
    line = json.loads(lines[-1])
    assert line["n_gpus"] == 2 and line["steps"] == 20 and line["warmup"] == 5 and line["scaling"] == "weak"
    assert line["config"]["global_boards"] == 2 * line["config"]["boards_per_gpu"] == 2 << 20
    t = line["timing"]
    # (no speed bar: two ranks share one GPU and gloo moves the exchange through host copies -- 4 MiB per rank with
    #  --gather full; the launch trains themselves must still be device-speed)
    assert t["collective_us"] > 0 and 0 < t["launch_train_us"] < 20 * 1000 and line["value"] > 1e7
    assert line["episodes_finished"] > 0
    if gather == "summary":
        g = line["global_returns"]                      # both ranks' summaries arrived: twice rank 0's shard, roughly
        assert 1.8 * line["episodes_finished"] < g["episodes"] < 2.2 * line["episodes_finished"]
    print(f"self-launched 2 ranks ({gather}): {line['value']:.3e} env-steps/s, timing {t}")


def test_bench_under_torch_distributed_run(torch_cuda):
    """The OTHER launch form of the contract -- `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr
    127.0.0.1 --master-port P bench.py --gpus N --steps K --warmup W` -- with N = 2 on the one GPU (both ranks on cuda:0, gloo):
    the launcher's RANK / LOCAL_RANK / WORLD_SIZE are used as they come, all ranks share one stdout and rank 0's JSON line must
    still be its LAST line."""
    import json
    import socket
    env = dict(os.environ, G2048_BENCH_BACKEND="gloo", G2048_BENCH_SAME_DEVICE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "G2048_BENCH_FORCE_DIST"):
        env.pop(k, None)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "20", "--warmup", "5",
           "--no-extras", "--boards", "131072", "--device-warmup", "0.05"]
    res = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = res.stdout.strip().splitlines()
    assert lines[-1].startswith("{"), lines[-3:]
    line = json.loads(lines[-1])
    cfg = line["config"]
    assert line["n_gpus"] == 2 and cfg["pg_world_size"] == 2 and cfg["gathered_rows"] == 2 and cfg["backend"] == "gloo"
    assert cfg["global_boards"] == 2 * 131072 and cfg["chains"] == 1 and line["value"] > 1e7


def test_bench_gpus_4_rehearsal_on_one_device(torch_cuda):
    """The driver's multi-GPU scaling command -- `python bench.py --gpus N --steps 20 --warmup 5` -- rehearsed end to end on
    the one GPU there is: four processes on cuda:0 (G2048_BENCH_SAME_DEVICE=1), gloo carrying the collectives (RCCL
    refuses two ranks on one device), 2^17 boards per rank.  Four, not the eight of a full node: a shared MI355X takes at
    most six processes with the device open, and this test's own process is one of them (the eight-rank rendezvous and
    relay run without a GPU: test_bench_helpers.py::test_launcher_rendezvous_of_eight_ranks).  What this pins: the
    rendezvous of the ranks, the relay of rank 0's JSON as the LAST line, exit code 0, a wall time far inside the driver's
    1 800 s -- and that the line describes itself: backend, the process group's world size, one gathered row per rank, the
    launch form (one chain at K = 20, as at N = 1)."""
    import json
    import time
    ranks = 4
    env = dict(os.environ, G2048_BENCH_BACKEND="gloo", G2048_BENCH_SAME_DEVICE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "G2048_BENCH_FORCE_DIST"):
        env.pop(k, None)
    t0 = time.time()
    res = _run_bench(["--gpus", str(ranks), "--steps", "20", "--warmup", "5", "--no-extras", "--boards", "131072",
                      "--device-warmup", "0.05"], env)
    took = time.time() - t0
    lines = res.stdout.strip().splitlines()
    assert lines[-1].startswith("{"), lines[-3:]
    line = json.loads(lines[-1])
    cfg = line["config"]
    assert line["n_gpus"] == ranks and line["steps"] == 20 and line["warmup"] == 5 and line["scaling"] == "weak"
    assert cfg["backend"] == "gloo" and cfg["pg_world_size"] == ranks and cfg["gathered_rows"] == ranks
    assert cfg["global_boards"] == ranks * cfg["boards_per_gpu"] == ranks * 131072
    assert cfg["chains"] == 1 and cfg["chains_requested"] == 1
    g = line["global_returns"]
    assert 0.75 * ranks * line["episodes_finished"] < g["episodes"] < 1.25 * ranks * line["episodes_finished"]   # every shard's worth
    assert line["value"] > 1e7 and len(line["timing"]["k_region_repeats_us"]) == 5
    assert took < 600, f"the {ranks}-rank rehearsal took {took:.0f} s"
    print(f"{ranks}-rank rehearsal on one device: {took:.0f} s wall, value {line['value']:.3e}, timing {line['timing']}")


def test_bench_dump_outputs_are_the_oracle_after_the_timed_steps(torch_cuda, tmp_path):
    """`bench.py --dump-outputs DIR` writes what the LAST timed step left its caller -- its reward and terminated rows, the
    boards and their scores -- for the fixed sample of boards bench.dump_sample picks (2^19 boards: a real sample), and
    that is exactly the C oracle after the same seeded steps: the AGE_STEPS fused ones, the W warm-up steps and the K timed
    ones (K = 200: the two-chain form).  The inputs are fixed by the arguments, so two builds compare output for output."""
    import json
    import bench
    from oracle import OracleBatch
    n, k, w = 1 << 19, 200, 5
    env = dict(os.environ)
    for key in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "G2048_BENCH_FORCE_DIST",
                "G2048_BENCH_SAME_DEVICE", "G2048_BENCH_BACKEND"):
        env.pop(key, None)
    out = tmp_path / "dump"
    res = _run_bench(["--steps", str(k), "--warmup", str(w), "--boards", str(n), "--no-extras", "--device-warmup", "0.05",
                      "--dump-outputs", str(out)], env)
    line = json.loads(res.stdout.strip().splitlines()[-1])
    assert line["steps"] == k and line["warmup"] == w and line["config"]["chains_requested"] == 2
    got = {p.stem: np.load(p) for p in out.glob("*.npy")}
    assert sorted(got) == ["board_index", "boards", "reward", "score", "terminated"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values()) and sum(a.nbytes for a in got.values()) <= 64 << 20
    idx = bench.dump_sample(n)
    assert len(idx) == bench.DUMP_SAMPLE < n and np.array_equal(got["board_index"], idx)
    ora = OracleBatch(n, bench.SEED, threads=0)
    ora.reset()
    for _ in range(bench.AGE_STEPS + w + k):
        ora.step(None)
    assert np.array_equal(got["reward"], ora.reward[idx])
    assert np.array_equal(got["terminated"], ora.terminated[idx]) and got["terminated"].any()
    assert np.array_equal(got["boards"].reshape(-1, 16), ora.boards[idx])
    assert np.array_equal(got["score"], ora.score[idx])


def test_policy_loop_bench_small(torch_cuda):
    """bench_policy.run (BASELINE configs[4] as bench.py's extras.policy_loop measures it) on a small batch: one env
    launch per step that reads the policy's int64 actions and writes the next fp16 observation, no host copies."""
    import bench_policy
    r = bench_policy.run(boards=8192, steps=2, warmup=1, chunk=4096)
    assert r["boards"] == 8192 and r["host_copies"] == 0 and r["launches_per_env_step"] == 1
    assert r["value"] > 0 and r["ms_per_step"]["env_step_with_observation"] > 0 and r["episodes_finished"] >= 0


def test_more_than_4_gib_of_records(torch_cuda):
    """2^28 + 4133 boards = 4 GiB + of records in ONE engine (the layout is sized for 288 GB): byte offsets of
    the records, the terminal records and the [K][N] float rewards exceed 32 bits.  Sharding invariance makes
    the check cheap: windows at the start, across the 4 GiB line and at the end must play exactly the games
    of small engines created with the same global board offsets, which in turn are checked against the oracle."""
    torch = torch_cuda
    from gym2048_amd.batched import Batched2048
    from oracle import OracleBatch
    n, seed, k, win = (1 << 28) + 4096 + 37, 5, 12, 2048
    big = Batched2048(n, seed=seed)
    big.reset()
    offsets = [0, (1 << 28) - win // 2, n - win]
    small = [Batched2048(win, seed=seed, board_offset=o) for o in offsets]
    oracles = [OracleBatch(win, seed, o, threads=0) for o in offsets]
    for e in small + oracles:
        e.reset()
    reward = torch.zeros((2, n), dtype=torch.float32, device=big.device)      # row 1 starts beyond 1 GiB, ends beyond 2 GiB
    for s in range(k):
        big.rollout(1, reward=reward[1:2])
        for e in small + oracles:
            e.step(None)
        recs = big.records()
        for o, e, ora in zip(offsets, small, oracles):
            assert torch.equal(recs[o:o + win], e.records()), (s, o)
            assert np.array_equal(reward[1, o:o + win].cpu().numpy(), ora.reward), (s, o)
            assert np.array_equal((e.records().cpu().numpy() & 0x1F), ora.boards), (s, o)
    assert big.clock == k
    last = big.last_records()
    for o, e, ora in zip(offsets, small, oracles):
        assert torch.equal(last[o:o + win], e.last_records())
        assert np.array_equal(e.get_last_scores(), ora.last_score)
    st = big.episode_stats()
    assert st["episodes"] > n // 2 and sum(st["highest_hist"]) == n
    big.close()


def test_numpy_rng_mode_at_scale_and_with_every_board_resetting(torch_cuda):
    """numpy-RNG mode compacts the boards that finished into per-wavefront lists and resets them in a second
    kernel.  (1) 2^18 boards x 20 steps of the synthetic policy against the oracle's numpy mode (RNG states
    included); (2) the worst case for the lists: EVERY board makes an illegal move in the same step (64 entries
    per wavefront, 1 024 per list group), with a ragged board count."""
    torch = torch_cuda
    from gym2048_amd.batched import Batched2048
    from oracle import OracleBatch
    n, seed = 1 << 18, 9
    eng = Batched2048(n, seed=seed, rng="numpy")
    ob = OracleBatch(n, seed, threads=0)
    ob.seed_numpy(seed)
    eng.reset()
    ob.reset_numpy()
    for s in range(20):
        eng.step(None)
        ob.step_numpy(None)
        assert np.array_equal(eng.reward.cpu().numpy(), ob.reward), s
        assert np.array_equal(eng.terminated.cpu().numpy(), ob.terminated), s
    assert np.array_equal(eng.get_boards().reshape(n, 16), ob.boards) and np.array_equal(eng.get_scores(), ob.score)
    assert np.array_equal(eng.get_numpy_rng().T, ob.rng) and np.array_equal(eng.get_last_scores(), ob.last_score)
    # (2) tiles packed against the top edge: "up" is illegal for every board
    n2 = 70000 + 37
    eng2 = Batched2048(n2, seed=seed + 1, rng="numpy", illegal_move_reward=-2.0)
    ob2 = OracleBatch(n2, seed + 1, threads=0)
    ob2.illegal_move_reward = -2.0
    ob2.seed_numpy(seed + 1)
    eng2.reset()
    ob2.reset_numpy()
    stuck = np.zeros((n2, 16), np.uint8)
    stuck[:, :4] = (1, 2, 3, 4)
    stuck[:, 4] = np.arange(n2) % 5                      # some variety below the top row (still no upward move)
    stuck[stuck[:, 4] == 1, 4] = 2                       # (a 2 under a 2 would merge upwards)
    eng2.set_boards(stuck)
    ob2.boards[:] = stuck
    up = np.zeros(n2, np.uint8)
    eng2.step(torch.as_tensor(up))
    ob2.step_numpy(up)
    assert ob2.terminated.all() and ob2.illegal.all()
    assert np.array_equal(eng2.terminated.cpu().numpy(), ob2.terminated) and (eng2.reward.cpu().numpy() == -2.0).all()
    assert np.array_equal(eng2.get_boards().reshape(n2, 16), ob2.boards)
    assert np.array_equal(eng2.get_numpy_rng().T, ob2.rng)
    assert (eng2.get_scores() == 0).all() and eng2.episode_stats()["illegal_ends"] == n2
    for s in range(6):                                   # and play on from there
        eng2.step(None)
        ob2.step_numpy(None)
    assert np.array_equal(eng2.get_boards().reshape(n2, 16), ob2.boards) and np.array_equal(eng2.get_numpy_rng().T, ob2.rng)
