"""Cost of mixed-length n-tuple networks (redundant encoding) on MI355X; appends to profiles/r18_ntuple_mixed_probe.txt.

Microseconds per launch (HIP events, two warm-up calls) of values, evaluate, search depth 1 (2^16 boards only), update and
tc_update (W + A) at 2^16 and 2^20 mid-game boards (200 random moves from the start), for
  (a) the uniform "4x6" network -- run once per library: ``--lib`` names another build (the parent commit's), so the uniform
      entry points at this commit stand next to the parent's, and two runs of one library give the spread to read the
      difference against;
  (b) the mixed "4x6+4x4" network;
  (c) the uniform T = 8, L = 6 network a user had to declare without mixed lengths: the 4x6 lists and four 6-tuples that
      contain the four 4-tuples;
  (d) the uniform network of the four 4-tuples alone: (a) and (d) together do the look-ups of (b), on the uniform kernels.
The variants alternate within one process, REPEATS rounds; every figure is the median of the rounds with the lowest and the
highest next to it.  With ``--lib`` only (a) runs: a build from before this feature refuses (b).  ``--uniform-only`` runs
only (a) on this build too: the same process as a ``--lib`` run, so the two compare like for like.

  python tools/ntuple_mixed_probe.py [--out FILE] [--lib PATH] [--uniform-only] [--tag TEXT]
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

from ntuple_probe import timed  # noqa: E402

SIZES, SEARCH_SIZES = (1 << 16, 1 << 20), (1 << 16,)
REPEATS = 5
# (c): the 4x6 lists, and the four 4-tuples of "4x6+4x4" each grown to six cells
TUPLES_8x6 = ((0, 1, 2, 3, 4, 5), (4, 5, 6, 7, 8, 9), (0, 1, 2, 4, 5, 6), (4, 5, 6, 8, 9, 10),
              (0, 1, 2, 3, 6, 7), (4, 5, 6, 7, 10, 11), (0, 1, 4, 5, 8, 9), (5, 6, 9, 10, 13, 14))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_ntuple_mixed_probe.txt"))
    ap.add_argument("--lib", default=None, help="another build of the library (the parent commit's) to time instead: part (a) only")
    ap.add_argument("--uniform-only", action="store_true", help="part (a) only on this build: the process of a --lib run")
    ap.add_argument("--tag", default="", help="a label for the header line")
    args = ap.parse_args()

    def say(line=""):
        print(line, flush=True)
        with open(args.out, "a") as f:                  # appended: one file holds the runs of both libraries
            f.write(line + "\n")

    import torch

    import gym2048_amd as g
    from gym2048_amd import _lib
    from gym2048_amd.ntuple import TUPLES
    if args.lib:
        _lib.LIB_PATH = args.lib
    else:
        import __graft_entry__ as ge
        ge.build()
    say(f"\n== {args.tag or 'run'}: {torch.cuda.get_device_name(0)}; library {os.path.basename(_lib.LIB_PATH)}"
        f"{' (--lib)' if args.lib else ''}; us per launch, median of {REPEATS} rounds [lowest .. highest]")
    eng = g.Batched2048(max(SIZES), seed=7)
    try:
        eng.reset()
        eng.rollout_random(200)
        played = eng.boards().reshape(-1, 16).clone()
    finally:
        eng.close()
    gen = torch.Generator(device="cuda").manual_seed(1)
    variants = [("(a) 4x6", "4x6")]
    if not args.lib and not args.uniform_only:
        variants += [("(b) 4x6+4x4", "4x6+4x4"), ("(c) 8x6", TUPLES_8x6), ("(d) 4x4", TUPLES["4x6+4x4"][4:])]
    nets = []
    for label, tuples in variants:
        net = g.NTupleNet(tuples)
        net.weights.random_(-(1 << 16), 1 << 16, generator=gen)
        nets.append((label, net, g.NTupleTC(net)))
        say(f"{label:12s} T = {net.n_tuples}, weights {net.weights.numel() * 4 / 2**20:.0f} MiB, TC accumulators "
            f"{net.weights.numel() * 16 / 2**20:.0f} MiB")

    for n in SIZES:
        boards = played[:n].contiguous()
        delta = torch.randint(-(1 << 20), 1 << 20, (n,), generator=gen, device="cuda", dtype=torch.int64) | 1
        times = {}
        for _ in range(REPEATS):                         # the variants alternate: a drift of the machine reaches all of them
            for label, net, tc in nets:
                calls = [("values", lambda: net.values(boards)), ("evaluate", lambda: net.evaluate(boards)),
                         ("update", lambda: net.update(boards, delta, 10)), ("tc_update", lambda: net.tc_update(boards, delta, 10, tc))]
                if n in SEARCH_SIZES:
                    calls.append(("search d1", lambda: net.search(boards, 1)))
                for name, fn in calls:
                    times.setdefault((name, label), []).append(timed(torch, fn, budget_ms=60.0))
        for (name, label), t in sorted(times.items()):
            t = sorted(t)
            say(f"n={n:8d} {name:10s} {label:12s} {t[REPEATS // 2]:10.1f} [{t[0]:9.1f} ..{t[-1]:9.1f}]")


if __name__ == "__main__":
    main()
