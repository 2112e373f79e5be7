"""Cost and strength of g2048_mc_search on MI355X.

Cost: microseconds per launch of g2048_mc_search_plain (HIP events) over n x R x L on mid-game boards (games played by
depth-1 expectimax, snapshots from move 100 on), and playout steps per second = (sum(steps) + legal roots * R) / time: the
moves played inside the playouts plus the root move of every playout.  Next to it the env-steps/s of
g2048_rollout_random on 2^20 boards in the same process, the engine's figure for one random step.

Strength: mean final score of GAMES games played to the end by the Monte-Carlo player for R in STRENGTH_R (playouts to
the end of the game), next to expectimax depth 1..3 and the random policy on the same engine seeds, with the time per
move (wall clock of the whole game loop over the moves played).

  python tools/mc_probe.py              # both tables
  python tools/mc_probe.py --quick      # one timed launch per cell, no games (for a rocprofv3 pass)
"""
from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]  # tests/analysis_helpers.py: play(), random_policy()

COST = [(1 << 12, 64, 65535), (1 << 12, 16, 65535), (1 << 16, 64, 65535), (1 << 16, 16, 65535), (1 << 16, 64, 32),
        (1 << 16, 16, 32), (1 << 16, 256, 65535), (1 << 20, 16, 32)]
STRENGTH_R = (4, 16, 64, 256)
GAMES = 512


def midgame_boards(g, torch, n_max):
    games = 4096
    eng = g.Batched2048(games, seed=1)
    out = torch.empty((n_max // games, games, 16), dtype=torch.uint8, device="cuda")
    try:
        eng.reset()
        for t in range(100 + n_max // games):
            if t >= 100:
                out[t - 100].copy_(eng.boards().reshape(games, 16))
            eng.step(eng.expectimax(1).action)
    finally:
        eng.close()
    return out.reshape(-1, 16).contiguous()


def time_launches(g, torch, boards, R, L, out, quick):
    for _ in range(1 if quick else 2):
        g.mc_search(boards, R, L, seed=1, out=out)
    torch.cuda.synchronize()
    reps, spent = 0, 0.0
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    while reps < (1 if quick else 3) or (not quick and spent < 300.0 and reps < 50):
        start.record()
        g.mc_search(boards, R, L, seed=1, out=out)
        end.record()
        end.synchronize()
        spent += start.elapsed_time(end)
        reps += 1
    return spent * 1e3 / reps  # us per launch


def rollout_random_rate(g, torch):
    n, k = 1 << 20, 1000
    eng = g.Batched2048(n, seed=3)
    try:
        eng.reset()
        eng.rollout_random(k)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.rollout_random(k)
        torch.cuda.synchronize()
        return n * k / (time.perf_counter() - t0)
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    import torch

    import __graft_entry__ as ge
    ge.build()
    import gym2048_amd as g
    from analysis_helpers import play, random_policy
    from gym2048_amd.transitions import mc_step_seed

    boards_all = midgame_boards(g, torch, 1 << 20)
    torch.cuda.synchronize()
    print(f"device: {torch.cuda.get_device_name(0)}")
    if not args.quick:
        print(f"g2048_rollout_random, 2^20 boards x 1000 steps: {rollout_random_rate(g, torch):.4g} env-steps/s")
    print("       n      R      L lanes/board   us/launch  playout steps/launch  playout steps/s  moves/playout")
    for n, R, L in COST:
        boards = boards_all[:n]
        out = g.MCSearch(torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty((n, 4), dtype=torch.int64, device="cuda"),
                         torch.empty((n, 4), dtype=torch.int64, device="cuda"))
        us = time_launches(g, torch, boards, R, L, out, args.quick)
        legal = out.steps >= 0
        playouts = int(legal.sum()) * R
        steps = int(out.steps[legal].sum()) + playouts
        print(f"{n:8d} {R:6d} {L:6d} {64 if R >= 32 else 16:11d} {us:11.1f} {steps:21d} {steps / us * 1e6:16.4g} "
              f"{(steps - playouts) / playouts:14.1f}", flush=True)
    if args.quick:
        return
    print(f"\n{GAMES} games to the end (numpy-RNG engine, seed 2048)")
    print("player            mean score   median      max  mean moves  us/move (whole batch)  us/move/board")
    players = [("random", random_policy(torch, GAMES, 2048))]
    players += [(f"expectimax d={d}", lambda e, t, d=d: e.expectimax(d).action) for d in (1, 2, 3)]
    players += [(f"mc R={R}", lambda e, t, R=R: e.mc_search(R, seed=mc_step_seed(2048, t)).action) for R in STRENGTH_R]
    for name, choose in players:
        score, _, moves, secs = play(g, torch, GAMES, 2048, choose, cap=20000)
        import numpy as np
        done = score >= 0
        print(f"{name:16s} {score[done].mean():11.1f} {np.median(score[done]):8.0f} {score[done].max():8d} {moves / GAMES:11.1f} "
              f"{secs * 1e6 / max(1, moves) * GAMES:22.1f} {secs * 1e6 / max(1, moves):14.3f}"
              + ("" if done.all() else f"   ({(~done).sum()} games unfinished at the move cap)"), flush=True)


if __name__ == "__main__":
    main()
