"""Cost of the multi-stage n-tuple network on MI355X; writes profiles/r15_ntuple_staged_probe.txt.

Part (a), the unstaged entry points: microseconds per call (HIP events) of values, evaluate, update, tc_update (W + A),
trace_update and tc_trace_update (H = 4, lambda = 0.5) and search depth 2 with an unstaged net on both default shapes and on an 8x4 net (T = 8,
the tuple count at its limit), at 1 024, 2^16 and 2^20 boards (search: 1 024 and 2^16).  Run once per library -- ``--lib`` names another build (the parent commit's) -- and compare the
tables: every figure is the median of REPEATS timings, printed with their lowest and highest, so the run-to-run spread of
each library is on the page next to the difference between the two.
Part (b), ``--staged``: the same calls with S = 4 (thresholds "has a 4", "has an 8", "has a 16 and an 8": boards after 200
random moves populate every stage) next to the unstaged net in the same process.

  python tools/ntuple_staged_probe.py [--out FILE] [--lib PATH] [--staged] [--tag TEXT]
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

from ntuple_probe import timed  # noqa: E402

SIZES, SEARCH_SIZES = (1 << 10, 1 << 16, 1 << 20), (1 << 10, 1 << 16)
# the two default shapes, and T = 8 at L = 4: the five 4-tuples of "17x4", an L, an S and a T shape
SHAPES = {"17x4": "17x4", "4x6": "4x6",
          "8x4": ((0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 4, 5), (1, 2, 5, 6), (5, 6, 9, 10), (0, 1, 2, 4), (0, 1, 5, 6), (0, 1, 2, 5))}
REPEATS = 5
DEPTH, LAM = 4, 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_ntuple_staged_probe.txt"))
    ap.add_argument("--lib", default=None, help="another build of the library (the parent commit's) to time instead")
    ap.add_argument("--staged", action="store_true", help="part (b): S = 4 next to the unstaged net")
    ap.add_argument("--tag", default="", help="a label for the header line")
    args = ap.parse_args()

    def say(line=""):
        print(line, flush=True)
        with open(args.out, "a") as f:                  # appended: one file holds the runs of both libraries
            f.write(line + "\n")

    import torch

    import gym2048_amd as g
    from gym2048_amd import _lib, ntuple
    if args.lib:
        _lib.LIB_PATH = args.lib                        # a build from before the staged symbols existed: bind what it has
        _lib.SIGNATURES = {k: v for k, v in _lib.SIGNATURES.items() if "_staged_" not in k and k != "g2048_ntuple_stage_plain"}
    else:
        import __graft_entry__ as ge
        ge.build()
    say(f"\n== {args.tag or 'run'}: {torch.cuda.get_device_name(0)}; library {os.path.basename(_lib.LIB_PATH)}; us per call, "
        f"median of {REPEATS} timings [lowest .. highest]")
    eng = g.Batched2048(max(SIZES), seed=7)
    try:
        eng.reset()
        eng.rollout_random(200)
        played = eng.boards().reshape(-1, 16).clone()
    finally:
        eng.close()
    gen = torch.Generator(device="cuda").manual_seed(1)
    thr = (ntuple.stage_mask(4), ntuple.stage_mask(8), ntuple.stage_mask(16, 8))

    def med(fn):
        t = sorted(timed(torch, fn, budget_ms=60.0) for _ in range(REPEATS))
        return f"{t[REPEATS // 2]:10.1f} [{t[0]:9.1f} ..{t[-1]:9.1f}]"

    def calls(net, n, boards):
        delta = torch.randint(-(1 << 20), 1 << 20, (n,), generator=gen, device="cuda", dtype=torch.int64) | 1
        tc, tr = g.NTupleTC(net), g.NTupleTrace(n, depth=DEPTH, lam=LAM)
        zero = torch.zeros(n, dtype=torch.int64, device="cuda")
        for k in range(DEPTH):                          # every board with a full history
            tr.push(boards.roll(k, 0).contiguous(), zero, zero, torch.zeros(n, dtype=torch.uint8, device="cuda"), zero.clone())
        out = [("values", lambda: net.values(boards)), ("evaluate", lambda: net.evaluate(boards)),
               ("update", lambda: net.update(boards, delta, 10)), ("tc_update", lambda: net.tc_update(boards, delta, 10, tc)),
               ("trace_update", lambda: net.trace_update(tr, delta, 10)),
               ("tc_trace_upd", lambda: net.tc_trace_update(tr, delta, 10, tc))]
        if n in SEARCH_SIZES:
            out.append(("search d2", lambda: net.search(boards, 2)))
        return out

    for shape, tuples in SHAPES.items():
        for n in SIZES:
            boards = played[:n].contiguous()
            nets = [("unstaged", g.NTupleNet(tuples))]
            if args.staged:
                nets.append(("S = 4", g.NTupleNet(tuples, stages=thr)))
                hist = torch.bincount(nets[1][1].stage(boards).long(), minlength=4).tolist()
                say(f"{shape} n={n}: boards per stage {hist}")
            for label, net in nets:
                net.weights.random_(-(1 << 16), 1 << 16, generator=gen)
                for name, fn in calls(net, n, boards):
                    say(f"{shape:5s} n={n:8d} {label:9s} {name:13s} {med(fn)}")
            del nets, net
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
