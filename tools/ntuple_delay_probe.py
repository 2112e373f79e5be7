"""Cost and learning curves of the n-tuple delay, delayed TD(lambda) and TC(lambda), on MI355X; writes
profiles/r22_ntuple_delay_probe.txt.

The histories come from real play: 2^20 boards 200 random steps into their games, then twelve greedy steps under the network
whose update is timed (evaluate, step with auto-reset, evaluate); the afterstates, values and flags of the last H steps are
pushed into a trace and into a delay ring, so both hold the same boards and the atomics collide as they do in training.
Push:     us per g2048_ntuple_delay_push next to g2048_ntuple_trace_push (HIP events), 1 024 and 2^20 boards, H = 4 and 8.
Update:   us per STEP update at H = 1, 2, 4, 8 next to the trace update of the same history and the one-step update of the
          newest afterstates, TD and TC (W + A), "4x6" and "4x6+4x4", 1 024 and 2^20 boards.  An update leaves its ring alone, so
          a call repeats exactly; the tables drift, as they do in training.
Training: ``--train``: 50 000 steps on 1 024 boards from zero weights, TC(lambda = 0.5, H = 4) (tcl_train) and delayed
          TC(lambda = 0.5, H = 4) (delayed_tcl_train), lr_shift 5, both networks: wall time, and the mean score of 512 greedy
          games (play_games) after every 10 000 steps.  One seed: the scores are reported, not compared.
``--lib PATH`` times another build of the library (the parent commit's): the trace and one-step rows only -- the baseline.

  python tools/ntuple_delay_probe.py [--out FILE] [--append] [--lib PATH] [--tag TEXT] [--no-cost] [--train] [--steps N]
"""
from __future__ import annotations

import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

from ntuple_probe import timed  # noqa: E402

SIZES = (1 << 10, 1 << 20)
DEPTHS = (1, 2, 4, 8)
SHAPES = ("4x6", "4x6+4x4")
BOARDS, STEPS, EVERY, GAMES = 1024, 50000, 10000, 512
LAM, DEPTH, TD_SHIFT, TC_SHIFT = 0.5, 4, 10, 5
PLAYED = 12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_ntuple_delay_probe.txt"))
    ap.add_argument("--append", action="store_true", help="keep what --out holds and write below it")
    ap.add_argument("--lib", default=None, help="another build of the library (the parent commit's): trace and one-step rows only")
    ap.add_argument("--tag", default="", help="a label for the header line")
    ap.add_argument("--no-cost", action="store_true")
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--steps", type=int, default=STEPS)
    args = ap.parse_args()
    rows = open(args.out).read().splitlines() if args.append and os.path.exists(args.out) else []

    def say(line=""):
        print(line, flush=True)
        rows.append(line)
        with open(args.out, "w") as f:      # kept current: a run that is cut short leaves what it measured
            f.write("\n".join(rows) + "\n")

    import torch

    from gym2048_amd import _lib
    if args.lib:
        other = ctypes.CDLL(args.lib)
        for name in [n for n in _lib.SIGNATURES if not hasattr(other, n)]:
            del _lib.SIGNATURES[name]      # a build from before this feature lacks the delay symbols
        _lib.LIB_PATH = args.lib
    else:
        import __graft_entry__ as ge
        ge.build()
    import gym2048_amd as g
    from gym2048_amd.ntuple import td_evaluate, td_work

    ours = not args.lib
    say(f"== {args.tag or 'run'}: {torch.cuda.get_device_name(0)}; library {os.path.basename(_lib.LIB_PATH)}{' (--lib)' if args.lib else ''}")

    def played(net, n):
        """The (after, after_value, best_next, terminated, delta) of the last 8 of PLAYED greedy steps of n mid-game boards."""
        eng = g.Batched2048(n, seed=7)
        try:
            eng.reset()
            eng.rollout_random(200)
            work, out = td_work(eng), []
            for _ in range(PLAYED):
                td_evaluate(eng, net, work)
                out.append((work.before.after.clone(), work.before.after_value.clone(), work.after.best.clone(),
                            eng.terminated.clone().to(torch.uint8), work.delta.clone()))
            return out[-8:]
        finally:
            eng.close()

    def rings(n, H, steps):
        tr = g.NTupleTrace(n, depth=H, lam=LAM)
        dl = g.NTupleDelay(n, depth=H, lam=LAM) if ours else None
        out = torch.empty(n, dtype=torch.int64, device="cuda")
        for after, av, bn, term, _ in steps:
            tr.push(after, av, bn, term, out)
            if ours:
                dl.push(after, av, bn, term, out)
        return tr, dl

    if not args.no_cost:
        say("\npush: us per call (HIP events), lambda = 0.5; the inputs are the last step of the play above under the zero 4x6 network")
        say("      n  H  trace push  delay push")
        net = g.NTupleNet("4x6")
        for n in SIZES:
            steps = played(net, n)
            after, av, bn, term, _ = steps[-1]
            for H in (4, 8):
                tr, dl = rings(n, H, steps)
                out = torch.empty(n, dtype=torch.int64, device="cuda")
                t_us = timed(torch, lambda: tr.push(after, av, bn, term, out))
                d_us = timed(torch, lambda: dl.push(after, av, bn, term, out)) if ours else float("nan")
                say(f"{n:7d} {H:2d} {t_us:11.1f} {d_us:11.1f}")
                del tr, dl
        del net
        torch.cuda.empty_cache()
        say("\nupdate: us per call (HIP events), lambda = 0.5.  one-step = update / tc_update of the newest afterstates with their delta;")
        say("trace = trace_update / tc_trace_update (up to H items per board); delay = delay_update / tc_delay_update in STEP mode (the")
        say("afterstates that leave the ring or whose episode ended, and a scan of len).  due = items a STEP update applies, of n.")
        say("TD lr_shift 10, TC lr_shift 5, W + A.  TC accumulators as 20 one-step updates left them.")
        say("shape          n  H      due  TD one-step  TD trace  TD delay  TC one-step  TC trace  TC delay")
        for shape in SHAPES:
            net = g.NTupleNet(shape)
            tc = g.NTupleTC(net)
            for n in SIZES:
                steps = played(net, n)
                after, _, _, _, delta = steps[-1]
                for r in range(20):
                    net.tc_update(after, delta.roll(r), TC_SHIFT, tc)
                td_us = timed(torch, lambda: net.update(after, delta, TD_SHIFT))
                tc_us = timed(torch, lambda: net.tc_update(after, delta, TC_SHIFT, tc, 3))
                for H in DEPTHS:
                    tr, dl = rings(n, H, steps)
                    tdl_us = timed(torch, lambda: net.trace_update(tr, delta, TD_SHIFT))
                    tcl_us = timed(torch, lambda: net.tc_trace_update(tr, delta, TC_SHIFT, tc, 3))
                    due = float("nan")
                    tdd_us = tcd_us = float("nan")
                    if ours:
                        ended = (dl.len & 0x80) != 0
                        L = (dl.len & 0x7f).clamp(max=H).to(torch.int64)
                        due = int(torch.where(ended, L, (L == H).to(torch.int64)).sum())
                        tdd_us = timed(torch, lambda: net.delay_update(dl, TD_SHIFT))
                        tcd_us = timed(torch, lambda: net.tc_delay_update(dl, TC_SHIFT, tc, 3))
                    say(f"{shape:8s} {n:7d} {H:2d} {due:8.0f} {td_us:12.1f} {tdl_us:9.1f} {tdd_us:9.1f} {tc_us:12.1f} {tcl_us:9.1f} {tcd_us:9.1f}")
                    del tr, dl
            del tc, net
            torch.cuda.empty_cache()
    if args.train and ours:
        say(f"\ntraining: {BOARDS} boards from zero weights (engine seed 11), H = {DEPTH}, lambda = {LAM}, lr_shift {TC_SHIFT}; after every {EVERY}")
        say(f"steps {GAMES} greedy games to the end (play_games on a {GAMES}-board engine, seed 2048).  One seed per row.")
        say("shape     learner            steps  train s  us/step  mean score  reach 2048  moves/game")
        for shape in SHAPES:
            for learner in ("TC(lam)", "delayed TC(lam)"):
                net = g.NTupleNet(shape)
                tc = g.NTupleTC(net)
                ring = g.NTupleTrace(BOARDS, depth=DEPTH, lam=LAM) if learner == "TC(lam)" else g.NTupleDelay(BOARDS, depth=DEPTH, lam=LAM)
                eng, judge = g.Batched2048(BOARDS, seed=11), g.Batched2048(GAMES, seed=2048)
                try:
                    eng.reset()
                    spent = 0.0
                    for done in range(0, args.steps + 1, EVERY):
                        if done:
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            if learner == "TC(lam)":
                                g.tcl_train(eng, net, tc, ring, EVERY, TC_SHIFT)
                            else:
                                g.delayed_tcl_train(eng, net, tc, ring, EVERY, TC_SHIFT)
                            torch.cuda.synchronize()
                            spent += time.perf_counter() - t0
                        judge.seed(2048)
                        rep = g.play_games(judge, net, games=1)
                        say(f"{shape:9s} {learner:16s} {done:7d} {spent:8.1f} {spent * 1e6 / max(1, done):8.1f} {rep.mean_score:11.1f} "
                            f"{rep.reach[2048]:11.4f} {rep.moves / max(1, rep.games):11.1f}")
                finally:
                    eng.close()
                    judge.close()
                del tc, net, ring
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
