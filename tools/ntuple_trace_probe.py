"""Cost and learning curves of the n-tuple traces, TD(lambda) and TC(lambda), on MI355X; writes
profiles/r14_ntuple_trace_probe.txt.

Push: microseconds per g2048_ntuple_trace_push launch (HIP events) next to the three torch element-wise launches it
replaces in td_evaluate (copy_, masked_fill_, sub_), at 1 024 and 2^20 boards.
Update: microseconds per trace update at H = 1, 2, 4, 8 (lambda = 0.5, every board with a full history and a non-zero delta
of mixed sign) next to the one-step update of the same boards: TD, and TC phases W + A, on the 17x4 net.
Learning: for each default shape, from zero weights on 1 024 boards, 50 000 steps of TD(0) (train, lr_shift 10), TD(lambda =
0.5, H = 4) (tdl_train, lr_shift 10), TC (tc_train, lr_shift 5) and TC(lambda = 0.5, H = 4) (tcl_train, lr_shift 5); after
every 10 000 steps the mean score of 512 greedy games.

  python tools/ntuple_trace_probe.py [--out FILE] [--no-curve] [--steps N]
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
DEPTHS = (1, 2, 4, 8)
SHAPES = ("17x4", "4x6")
BOARDS, STEPS, EVERY, GAMES = 1024, 50000, 10000, 512
LAM, DEPTH = 0.5, 4
RUNS = (("TD(0)", 10), ("TD(lam)", 10), ("TC", 5), ("TC(lam)", 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_ntuple_trace_probe.txt"))
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

    say("\npush: us per call (HIP events); torch = copy_, masked_fill_(terminated.bool()), sub_ as td_evaluate forms delta")
    say("      n  trace push (store board + len + delta)  torch, three launches")
    for n in SIZES:
        tr = g.NTupleTrace(n, depth=DEPTH, lam=LAM)
        after = played[:n].contiguous()
        av = torch.randint(-(1 << 20), 1 << 20, (n,), generator=gen, device="cuda", dtype=torch.int64)
        bn = torch.randint(-(1 << 20), 1 << 20, (n,), generator=gen, device="cuda", dtype=torch.int64)
        term = (torch.rand(n, generator=gen, device="cuda") < 0.01).to(torch.uint8)
        out = torch.empty(n, dtype=torch.int64, device="cuda")

        def three():
            out.copy_(bn)
            out.masked_fill_(term.bool(), 0)
            out.sub_(av)

        say(f"{n:7d} {timed(torch, lambda: tr.push(after, av, bn, term, out)):41.1f} {timed(torch, three):22.1f}")
        del tr
    say("\nupdate: us per call, 17x4 net, lambda = 0.5, every board with a full history of boards 200 random steps into their")
    say("games (the same board in every slot) and a non-zero delta of mixed sign; TC accumulators as 20 earlier updates left them")
    say("      n  H  TD trace  TD one-step  ratio  TC trace W + A  TC one-step W + A  ratio")
    net = g.NTupleNet("17x4")
    tc = g.NTupleTC(net)
    for n in SIZES:
        b = played[:n].contiguous()
        delta = torch.randint(-(1 << 14), 1 << 14, (n,), generator=gen, device="cuda", dtype=torch.int64) | 1
        for r in range(20):
            net.tc_update(b, delta.roll(r), 5, tc)
        td_us = timed(torch, lambda: net.update(b, delta, 5))
        tc_us = timed(torch, lambda: net.tc_update(b, delta, 5, tc, 3))
        for H in DEPTHS:
            tr = g.NTupleTrace(n, depth=H, lam=LAM)
            tr.hist.copy_(b.unsqueeze(0).expand(H, n, 16))
            tr.len.fill_(H)
            tdl_us = timed(torch, lambda: net.trace_update(tr, delta, 5))
            tcl_us = timed(torch, lambda: net.tc_trace_update(tr, delta, 5, tc, 3))
            say(f"{n:7d} {H:2d} {tdl_us:9.1f} {td_us:12.1f} {tdl_us / td_us:6.2f} {tcl_us:15.1f} {tc_us:18.1f} {tcl_us / tc_us:6.2f}")
            del tr
    del tc, net
    torch.cuda.empty_cache()
    if not args.no_curve:
        say(f"\nlearning: {BOARDS} boards from zero weights (engine seed 11), traces H = {DEPTH}, lambda = {LAM}; after every {EVERY}"
            f" steps {GAMES} greedy games to the end (numpy-RNG engine, seed 2048)")
        say("shape  learner  lr_shift    steps  train s  us/step  mean score  median     max  mean moves")
        for shape in SHAPES:
            for learner, shift in RUNS:
                net = g.NTupleNet(shape)
                tc = g.NTupleTC(net) if learner.startswith("TC") else None
                trace = g.NTupleTrace(BOARDS, depth=DEPTH, lam=LAM) if learner.endswith("(lam)") else None
                eng = g.Batched2048(BOARDS, seed=11)
                try:
                    eng.reset()
                    spent = 0.0
                    for done in range(0, args.steps + 1, EVERY):
                        if done:
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            if learner == "TD(0)":
                                g.train(eng, net, EVERY, shift)
                            elif learner == "TD(lam)":
                                g.tdl_train(eng, net, trace, EVERY, shift)
                            elif learner == "TC":
                                g.tc_train(eng, net, tc, EVERY, shift)
                            else:
                                g.tcl_train(eng, net, tc, trace, EVERY, shift)
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
                del tc, net, trace
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
