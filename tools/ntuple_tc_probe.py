"""Learning curves and cost of temporal-coherence learning on MI355X; writes profiles/r13_ntuple_tc_probe.txt.

Learning: for each default shape, from zero weights on 1 024 boards, 50 000 steps of (a) train() -- TD(0) at lr_shift 10,
the run of profiles/r11_ntuple_probe.txt repeated on this commit -- and (b) tc_train() at lr_shift 3, 5, 7 and 10 (a
weight's step is 2^-lr_shift * rate * delta and a value sums 8T = 32 or 40 weights, so 5 is about 1 / 8T); after every
10 000 steps the mean score of 512 greedy games.
Time: microseconds per launch (HIP events) of tc_update phase W, phase A and both, next to the TD(0) update of the same
boards and deltas, at 1 024 and 2^20 boards 200 random steps into their games.

  python tools/ntuple_tc_probe.py [--out FILE] [--no-curve] [--steps N]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]  # tests/analysis_helpers.py: play()

from ntuple_probe import timed  # noqa: E402

SIZES = (1 << 10, 1 << 20)
SHAPES = ("4x6", "17x4")
BOARDS, STEPS, EVERY, GAMES = 1024, 50000, 10000, 512
RUNS = (("td", 10), ("tc", 3), ("tc", 5), ("tc", 7), ("tc", 10))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_ntuple_tc_probe.txt"))
    ap.add_argument("--no-curve", action="store_true")
    ap.add_argument("--steps", type=int, default=STEPS)
    args = ap.parse_args()
    rows = []

    def say(line=""):
        print(line, flush=True)
        rows.append(line)
        with open(args.out, "w") as f:      # kept current: a run that is cut short leaves what it measured
            f.write("\n".join(rows) + "\n")

    import numpy as np
    import torch

    import __graft_entry__ as ge
    ge.build()
    import gym2048_amd as g
    from analysis_helpers import play

    say(f"device: {torch.cuda.get_device_name(0)}")
    eng = g.Batched2048(max(SIZES), seed=7)
    try:
        eng.reset()
        eng.rollout_random(200)
        played = eng.boards().reshape(-1, 16).clone()
    finally:
        eng.close()
    gen = torch.Generator(device="cuda").manual_seed(1)
    say("\nupdate: us per call, every delta non-zero and of mixed sign, boards 200 random steps into their games;")
    say("accumulators as 20 earlier tc updates of the same boards left them")
    say("shape       n  look-ups/board  tc W (loads + 32-bit atomics)  tc A (64-bit atomics)  tc W + A  TD(0) update  (W + A) / TD(0)")
    for shape in SHAPES:
        net = g.NTupleNet(shape)
        tc = g.NTupleTC(net)
        for n in SIZES:
            b = played[:n].contiguous()
            delta = torch.randint(-(1 << 14), 1 << 14, (n,), generator=gen, device="cuda", dtype=torch.int64) | 1
            for _ in range(20):
                net.tc_update(b, delta.roll(_), 5, tc)
            w_us = timed(torch, lambda: net.tc_update(b, delta, 5, tc, 1))
            a_us = timed(torch, lambda: net.tc_update(b, delta, 5, tc, 2))
            both_us = timed(torch, lambda: net.tc_update(b, delta, 5, tc, 3))
            td_us = timed(torch, lambda: net.update(b, delta, 5))
            say(f"{shape:5s} {n:7d} {8 * net.n_tuples:15d} {w_us:30.1f} {a_us:22.1f} {both_us:9.1f} {td_us:13.1f} {both_us / td_us:16.2f}")
        del tc, net
        torch.cuda.empty_cache()
    if not args.no_curve:
        say(f"\nlearning: {BOARDS} boards from zero weights (engine seed 11); after every {EVERY} steps {GAMES} greedy games to the"
            " end (numpy-RNG engine, seed 2048)")
        say("shape  learner  lr_shift    steps  train s  us/step  mean score  median     max  mean moves")
        for shape in SHAPES:
            for learner, shift in RUNS:
                net = g.NTupleNet(shape)
                tc = g.NTupleTC(net) if learner == "tc" else None
                eng = g.Batched2048(BOARDS, seed=11)
                try:
                    eng.reset()
                    spent = 0.0
                    for done in range(0, args.steps + 1, EVERY):
                        if done:
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            if tc is None:
                                g.train(eng, net, EVERY, shift)
                            else:
                                g.tc_train(eng, net, tc, EVERY, shift)
                            torch.cuda.synchronize()
                            spent += time.perf_counter() - t0
                        act = torch.empty(GAMES, dtype=torch.uint8, device="cuda")
                        pick = g.NTupleEval(None, act, None, None, None)
                        score, illegal, moves, _ = play(g, torch, GAMES, 2048, lambda e, t: e.ntuple_evaluate(net, out=pick).action,
                                                        cap=20000)
                        ok = score >= 0
                        say(f"{shape:5s} {learner:>7s} {shift:9d} {done:8d} {spent:8.1f} {spent * 1e6 / max(1, done):8.1f} "
                            f"{score[ok].mean():11.1f} {np.median(score[ok]):7.0f} {score[ok].max():7d} {moves / GAMES:11.1f}"
                            + (" (illegal pick!)" if illegal else "")
                            + ("" if ok.all() else f" ({(~ok).sum()} games unfinished at the cap)"))
                finally:
                    eng.close()
                del tc, net
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
