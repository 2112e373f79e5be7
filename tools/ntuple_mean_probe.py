"""Cost and learning of the batch-mean n-tuple update on MI355X; writes
profiles/r26_ntuple_mean_probe.txt.

Time: us per step (HIP events, steps alternating between the two forms in one build) of td_step (the summed update) and
mean_step at 1 024, 16 384, 65 536 and 2^20 boards for "4x6" and "4x6+4x4", and of the two new kernels alone (phases 1 and 2)
next to the summed update on the boards and errors of the last step.
Learning: "4x6", frac_bits 10, zero weights, engine seed 11, every run the same number of board-steps: the summed update at
1 024 boards with three neighbouring lr_shift; at 65 536 and 2^20 boards with the best of those and with three of its own; the
mean update at all three sizes with ONE lr_shift (three candidates, each run at all three sizes).  Each net is scored by
play_games at 1 024 boards, one game each (engine seed 2048): mean score and the share of games that reach 2048; wall time of
the training beside it.

  python tools/ntuple_mean_probe.py [--out FILE] [--no-time] [--no-learn] [--log2-board-steps K]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

SIZES = (1 << 10, 1 << 14, 1 << 16, 1 << 20)
SHAPES = ("4x6", "4x6+4x4")
SMALL, LARGE = 1 << 10, (1 << 16, 1 << 20)
SUM_SHIFTS_SMALL = (8, 10, 12)          # around the lr_shift 10 of the earlier probes at 1 024 boards
SUM_SHIFTS_LARGE = {1 << 16: (14, 16, 18), 1 << 20: (18, 20, 22)}   # the small batch's best, moved by log2 of the batch ratio
MEAN_SHIFTS = (4, 6, 8)                 # a value sums 8T = 32 weights: 5 moves V by the whole error; each is run at ALL sizes
GAMES = 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_ntuple_mean_probe.txt"))
    ap.add_argument("--no-time", action="store_true")
    ap.add_argument("--no-learn", action="store_true")
    ap.add_argument("--log2-board-steps", type=int, default=28)
    args = ap.parse_args()
    rows = []

    def say(line=""):
        print(line, flush=True)
        rows.append(line)
        with open(args.out, "w") as f:      # kept current: a run that is cut short leaves what it measured
            f.write("\n".join(rows) + "\n")

    import torch

    import gym2048_amd as g
    from gym2048_amd import _lib
    from gym2048_amd.ntuple import td_work
    from ntuple_probe import timed
    _lib.load()

    say(f"device: {torch.cuda.get_device_name(0)}")
    if not args.no_time:
        say("\ntime: us per call (HIP events); a step is evaluate, step, evaluate, three element-wise launches and the update;")
        say("weights as 300 TD(0) steps at lr_shift 10 left them, the two forms alternating call by call")
        say("shape          n  td_step  mean_step  mean/td   summed update  mean SUM  mean APPLY  SUM + APPLY")
        for shape in SHAPES:
            net = g.NTupleNet(shape)
            mean = g.NTupleMean(net)
            for n in SIZES:
                eng = g.Batched2048(n, seed=7)
                try:
                    eng.reset()
                    work = td_work(eng)
                    for _ in range(300):
                        g.td_step(eng, net, 10, work)
                    torch.cuda.synchronize()
                    td_us = mean_us = 0.0
                    for _ in range(3):                       # three rounds of each, interleaved
                        td_us += timed(torch, lambda: g.td_step(eng, net, 10, work), budget_ms=150.0) / 3
                        mean_us += timed(torch, lambda: g.mean_step(eng, net, mean, 10, work), budget_ms=150.0) / 3
                    b, d = work.before.after, work.delta
                    up_us = timed(torch, lambda: net.update(b, d, 10), budget_ms=100.0)
                    # SUM alone would pile up state: each timed call is SUM then APPLY, and APPLY alone runs on what SUM left
                    both_us = timed(torch, lambda: net.mean_update(b, d, 10, mean, 3), budget_ms=100.0)

                    def sum_only():
                        net.mean_update(b, d, 10, mean, 1)
                    sum_us = timed(torch, sum_only, budget_ms=100.0)
                    mean.reset()
                    say(f"{shape:8s} {n:8d} {td_us:8.1f} {mean_us:10.1f} {mean_us / td_us:8.2f} {up_us:15.1f} {sum_us:9.1f} "
                        f"{both_us - sum_us:11.1f} {both_us:12.1f}")
                finally:
                    eng.close()
            del mean, net
            torch.cuda.empty_cache()
        say("(mean APPLY = SUM + APPLY less SUM alone: APPLY alone on zero state would claim nothing)")
    if not args.no_learn:
        total = 1 << args.log2_board_steps
        say(f"\nlearning: \"4x6\", frac_bits 10, zero weights, engine seed 11, {total} board-steps per run (2^{args.log2_board_steps});")
        say(f"score: play_games, {GAMES} boards, 1 game each, engine seed 2048")
        say("update  boards  lr_shift     steps  train s  mean score  reach 2048  reach 4096")

        def run(kind, n, shift):
            net = g.NTupleNet("4x6", frac_bits=10)
            mean = g.NTupleMean(net) if kind == "mean" else None
            eng = g.Batched2048(n, seed=11)
            try:
                eng.reset()
                steps = total // n
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if mean is None:
                    g.train(eng, net, steps, shift)
                else:
                    g.mean_train(eng, net, mean, steps, shift)
                torch.cuda.synchronize()
                spent = time.perf_counter() - t0
            finally:
                eng.close()
            player = g.Batched2048(GAMES, seed=2048)
            try:
                rep = g.play_games(player, net, games=1, max_steps=1 << 17)
            finally:
                player.close()
            say(f"{kind:6s} {n:7d} {shift:9d} {steps:9d} {spent:8.1f} {rep.mean_score:11.1f} {rep.reach[2048]:11.4f} {rep.reach[4096]:11.4f}"
                + (f"  ({rep.unfinished} games unfinished)" if rep.unfinished else ""))
            del mean, net
            torch.cuda.empty_cache()
            return rep.mean_score

        best = max(SUM_SHIFTS_SMALL, key=lambda s: run("summed", SMALL, s))
        say(f"(the summed update's best lr_shift at {SMALL} boards: {best})")
        for n in LARGE:
            shifts = sorted(set((best,) + SUM_SHIFTS_LARGE[n]))
            for s in shifts:
                run("summed", n, s)
        for s in MEAN_SHIFTS:
            for n in (SMALL,) + LARGE:
                run("mean", n, s)


if __name__ == "__main__":
    main()
