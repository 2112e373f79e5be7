"""Cost of g2048_expectimax_plain on MI355X: microseconds per launch (HIP events), boards/s and leaves/s at depth 1, 2, 3
for n in {2^12, 2^16, 2^20} (depth 3 up to 2^16), on two board sets:

  mid-game  boards of games played by depth-1 expectimax (4 096 games, snapshots of steps 100 .. 100 + n / 4 096);
  random    boards of a uniform random-policy rollout (auto-reset; early-game boards with many empty cells).

A leaf is one heuristic evaluation.  Leaves per board are counted exactly on the host over a 1 024-board sample of each
set and scaled to n.  The host baseline is the same header (tests/host_check/host_check.cpp, g++ -O2) on one
thread over a sample, scaled to n; the ratio column is host time / kernel time.

  python tools/search_probe.py            # full table
  python tools/search_probe.py --quick    # one timed launch per cell, no host baseline (for a rocprofv3 pass)
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]  # tests/analysis_helpers.py: the host build of the search

SIZES = (1 << 12, 1 << 16, 1 << 20)
HOST_SAMPLE = {1: 4096, 2: 256, 3: 8}  # boards timed on the host per depth
LEAF_SAMPLE = 1024


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


def random_boards(g, torch, n_max):
    envs = 1 << 16
    eng = g.Batched2048(envs, seed=2)
    out = torch.empty((n_max // envs, envs, 16), dtype=torch.uint8, device="cuda")
    try:
        eng.reset()
        eng.rollout_random(20)
        for t in range(n_max // envs):
            eng.rollout_random(3)
            out[t].copy_(eng.boards().reshape(envs, 16))
    finally:
        eng.close()
    return out.reshape(-1, 16).contiguous()


def time_launches(g, torch, boards, depth, out, quick):
    for _ in range(1 if quick else 2):
        g.expectimax(boards, depth, out=out)
    torch.cuda.synchronize()
    reps, spent = 0, 0.0
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    while reps < (1 if quick else 3) or (not quick and spent < 200.0 and reps < 50):
        start.record()
        g.expectimax(boards, depth, out=out)
        end.record()
        end.synchronize()
        spent += start.elapsed_time(end)
        reps += 1
    return spent * 1e3 / reps  # us per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    import torch

    import __graft_entry__ as ge
    ge.build()
    import gym2048_amd as g

    from analysis_helpers import load_host_lib
    host = None if args.quick else load_host_lib()
    sets = {"mid-game": midgame_boards(g, torch, SIZES[-1]), "random": random_boards(g, torch, SIZES[-1])}
    torch.cuda.synchronize()
    print(f"device: {torch.cuda.get_device_name(0)}; weights: defaults {tuple(g.SearchWeights())}")
    print("set       depth        n   us/launch      boards/s      leaves/s  leaves/board  host us/board  host/kernel")
    for name, all_boards in sets.items():
        sample = np.ascontiguousarray(all_boards[:: all_boards.shape[0] // LEAF_SAMPLE][:LEAF_SAMPLE].cpu().numpy())
        empty = float((sample == 0).sum(1).mean())
        print(f"# {name}: mean empty cells {empty:.2f}, mean highest exponent {float(sample.max(1).mean()):.2f}")
        for depth in (1, 2, 3):
            leaves = None
            if host is not None:
                leaves = host.search_check_leaves(sample.ctypes.data, len(sample), depth) / len(sample)
                hs = sample[: HOST_SAMPLE[depth]]
                act, val = np.zeros(len(hs), np.uint8), np.zeros((len(hs), 4), np.int32)
                t0 = time.perf_counter()
                host.search_check_boards(hs.ctypes.data, len(hs), depth, (C.c_int32 * 4)(*g.SearchWeights()),
                                         act.ctypes.data, val.ctypes.data)
                host_us = (time.perf_counter() - t0) * 1e6 / len(hs)
                dev = g.expectimax(torch.as_tensor(hs).cuda(), depth)
                assert np.array_equal(dev.action.cpu().numpy(), act) and np.array_equal(dev.value.cpu().numpy(), val)
            for n in SIZES:
                if depth == 3 and n > (1 << 16):
                    continue
                boards = all_boards[:n]
                out = g.Search(torch.empty(n, dtype=torch.uint8, device="cuda"),
                               torch.empty((n, 4), dtype=torch.int32, device="cuda"))
                us = time_launches(g, torch, boards, depth, out, args.quick)
                line = f"{name:9s} {depth:5d} {n:8d} {us:11.1f} {n / us * 1e6:13.4g}"
                if leaves is not None:
                    line += f" {leaves * n / us * 1e6:13.4g} {leaves:13.1f} {host_us:14.2f} {host_us * n / us:12.0f}"
                print(line, flush=True)


if __name__ == "__main__":
    main()
