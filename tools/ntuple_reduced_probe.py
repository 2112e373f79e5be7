"""Cost of the n-tuple reduced search (g2048_ntuple_reduced_search) on MI355X; the results are kept in
profiles/r27_ntuple_reduced_probe.txt.  A launch is timed by HIP events after one warm-up launch, 15 launches per row, median
(min .. max).  Board sets and networks are those of tools/ntuple_adaptive_probe.py: the late-game set (1..4 empty cells), the
mid-game set (200 random moves in), the "4x6" and "4x6+4x4" networks with random weights, 1 024 boards.  The baseline of every row
is g2048_ntuple_adaptive_search at the same schedule on the same boards, its launches interleaved with the reduced search's.

(1) Constant schedules 2, 3 and 4 on the late-game set and 3 on the mid-game set, reduce4 = 1 and 2 next to the adaptive search:
    us per launch, the evaluations per board counted from the definition (a torch expansion of the tree's shape on a sample of 8
    of the same boards, checked against the pure-Python count of tests/ntuple_reduced_helpers.py on one board) and G evaluations
    per second -- what the units of unequal depth cost.
(2) The schedules "3-ply-late" and "4-ply-late" on a batch of 512 late-game and 512 mid-game boards (engine form).
(3) play_games at 256 boards, one game each, "4x6" after a short train() run, seed 2048, chunk 32: AdaptivePlayer("3-ply-late"),
    AdaptivePlayer("4-ply-late"), ReducedPlayer("4-ply-late", 1), ReducedPlayer("4-ply-late", 2) and ReducedPlayer(WIDE, 1), a
    wider schedule.  One sample on a briefly trained network: it says nothing firm about playing strength.

Every section runs in a child process of its own under its own time limit (SECTION_SECONDS); a section that fails or runs out
of time ends the run, and what was measured until then is kept.

  python tools/ntuple_reduced_probe.py [--out FILE] [--only 1,2,3] [--train-steps N] [--play-max-steps N] [--players 0,1,2,3,4]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]

from ntuple_adaptive_probe import N, adaptive_out, interleaved_us  # noqa: E402
from ntuple_deep_probe import PLAY_BOARDS, SHAPES, board_sets, random_net, sized, spread  # noqa: E402

# 4-ply up to 3 empty cells (the preset stops at 1), 3-ply up to 7 (5), 2-ply up to 11 (9), 1-ply above
WIDE = (4, 4, 4, 4, 3, 3, 3, 3, 2, 2, 2, 2, 1, 1, 1, 1, 1)


def evaluations_per_board(g, torch, boards, depth, R):
    """Mean network evaluations (legal leaf moves) per board of the depth-``depth`` tree with the children of a 4 spawn R plies
    shallower (R = 0: the adaptive search), counted from the definition on a sample in torch."""
    from ntuple_search_probe import children

    def count(frontier, k):
        if len(frontier) == 0:
            return 0
        if k == 0:
            legal = g.afterstates(frontier.contiguous()).legal
            return sum(((legal >> d) & 1).sum().item() for d in range(4))
        _, kids, weight, _, _ = children(g, torch, frontier.contiguous())
        four = max(k - 1 - R, 0)
        if four == k - 1:
            return count(kids, k - 1)
        return count(kids[weight == 9], k - 1) + count(kids[weight == 1], four)

    return count(boards, depth) / len(boards)


def check_the_count(g, torch, sample):
    """The torch count against the pure-Python count of the tests on the sample's first board."""
    from ntuple_reduced_helpers import evaluations
    one = sample[:1].contiguous()
    for depth, R in ((2, 1), (3, 0), (3, 1), (3, 2)):
        assert evaluations_per_board(g, torch, one, depth, R) == evaluations(one[0].cpu().numpy(), depth, R), (depth, R)


def report_constant(say, g, torch, sets, nets):
    say("(1) constant schedules, 1 024 boards, plain form: g2048_ntuple_adaptive_search (the baseline) and g2048_ntuple_reduced_search at reduce4 = 1, 2,")
    say("    launches interleaved; us per launch, median (min .. max; launches timed); evaluations per board counted from the definition on a sample")
    say("    of 8 of the same boards; G evaluations per second = 1 024 * evaluations / median")
    say("net       set   depth  search      evals/board   of adaptive   us per launch                                  Gevals/s   time / adaptive")
    for kind, depths in (("late", (2, 3, 4)), ("mid", (3,))):
        boards = sets[kind]
        sample = boards[:: max(1, len(boards) // 8)][:8].contiguous()
        if kind == "late":
            check_the_count(g, torch, sample)
        b = sized(boards, N)
        for depth in depths:
            evals = [evaluations_per_board(g, torch, sample, depth, R) for R in (0, 1, 2)]
            torch.cuda.empty_cache()
            for shape, net in nets.items():
                outs = [adaptive_out(g, torch, N) for _ in range(3)]
                sched = (depth,) * 17
                fns = [lambda: net.adaptive_search(b, sched, out=outs[0]), lambda: net.reduced_search(b, sched, 1, out=outs[1]),
                       lambda: net.reduced_search(b, sched, 2, out=outs[2])]
                us = interleaved_us(torch, fns)
                base = statistics.median(us[0])
                for name, e, t in zip(("adaptive", "reduce4=1", "reduce4=2"), evals, us):
                    m = statistics.median(t)
                    say(f"{shape:9s} {kind:5s} {depth:5d}  {name:10s} {e:12.4e}  {e / evals[0]:11.3f}   {spread(t)}  {N * e / m / 1e3:9.2f}   {m / base:10.3f}")


def report_schedules(say, g, torch, sets, nets):
    say("\n(2) the preset schedules on 512 late-game + 512 mid-game boards (engine form), launches interleaved; us per call")
    say("net       schedule      search      us per call                                     time / adaptive")
    boards = torch.cat([sized(sets["late"], N // 2), sized(sets["mid"], N // 2)]).contiguous()
    eng = g.Batched2048(N, seed=23)
    try:
        eng.set_boards(boards.cpu().numpy())
        for shape, net in nets.items():
            for schedule in ("3-ply-late", "4-ply-late"):
                outs = [adaptive_out(g, torch, N) for _ in range(3)]
                fns = [lambda: eng.ntuple_adaptive_search(net, schedule, out=outs[0]), lambda: eng.ntuple_reduced_search(net, schedule, 1, out=outs[1]),
                       lambda: eng.ntuple_reduced_search(net, schedule, 2, out=outs[2])]
                us = interleaved_us(torch, fns)
                assert torch.equal(outs[0].depth, outs[1].depth) and torch.equal(outs[0].depth, outs[2].depth)
                base = statistics.median(us[0])
                for name, t in zip(("adaptive", "reduce4=1", "reduce4=2"), us):
                    say(f"{shape:9s} {schedule:12s}  {name:10s}  {spread(t)}   {statistics.median(t) / base:10.3f}")
    finally:
        eng.close()


def report_games(say, g, torch, train_steps, max_steps, players):
    net = g.NTupleNet("4x6")
    trainer = g.Batched2048(1024, seed=11)
    try:
        trainer.reset()
        g.train(trainer, net, train_steps, 10)
    finally:
        trainer.close()
    say(f"\n(3) play_games at {PLAY_BOARDS} boards, one game each, \"4x6\" after train() of {train_steps} TD(0) steps on 1 024 boards, seed 2048, chunk 32"
        + (f", stopped after {max_steps} moves per board" if max_steps else "") + "; wall seconds of the call (device synchronised)")
    say("    One sample on a briefly trained network: it says nothing firm about playing strength.")
    say(f"    WIDE = {WIDE}")
    say("player                               seconds   games  unfinished  mean score    moves   moves/s   reach 2048 / 4096 / 8192")
    every = (("AdaptivePlayer(\"3-ply-late\")", lambda: g.AdaptivePlayer(net, "3-ply-late")),
             ("AdaptivePlayer(\"4-ply-late\")", lambda: g.AdaptivePlayer(net, "4-ply-late")),
             ("ReducedPlayer(\"4-ply-late\", 1)", lambda: g.ReducedPlayer(net, "4-ply-late", 1)),
             ("ReducedPlayer(\"4-ply-late\", 2)", lambda: g.ReducedPlayer(net, "4-ply-late", 2)),
             ("ReducedPlayer(WIDE, 1)", lambda: g.ReducedPlayer(net, WIDE, 1)))
    for name, make in [every[k] for k in players]:
        eng = g.Batched2048(PLAY_BOARDS, seed=2048)
        try:
            g.play_games(eng, net, games=1, chunk=4, max_steps=4, player=make())                          # warm-up
            eng.seed(2048)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rep = g.play_games(eng, net, games=1, chunk=32, max_steps=max_steps, player=make())
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        finally:
            eng.close()
        say(f"{name:34s} {dt:9.2f} {rep.games:7d} {rep.unfinished:11d} {rep.mean_score:11.1f} {rep.moves:8d} {rep.moves / dt:9.1f}   "
            f"{rep.reach[2048]:.3f} / {rep.reach[4096]:.3f} / {rep.reach[8192]:.3f}")


SECTION_SECONDS = {"1": 360, "2": 180, "3": 540}      # the time limit of each section's own process


def run_sections(args):
    """Every section in a child process of its own under its own time limit (a section that hangs or faults the GPU ends
    there: nothing is started after it); the children's outputs, in order, make ``args.out``."""
    import subprocess
    done = []
    for k in args.only.split(","):
        part = f"{args.out}.section{k}"
        cmd = [sys.executable, os.path.abspath(__file__), "--section", k, "--out", part, "--train-steps", str(args.train_steps),
               "--play-max-steps", str(args.play_max_steps), "--players", args.players]
        try:
            rc = subprocess.run(cmd, timeout=SECTION_SECONDS[k]).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if os.path.exists(part):
            with open(part) as f:
                text = f.read()
            os.remove(part)
            done.append(text if not done else text.split("\n", 1)[1])     # (the device line once)
            with open(args.out, "w") as f:
                f.write("".join(done))
        if rc != 0:
            print(f"section {k} ended with status {rc}: stopping", flush=True)
            return rc
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_ntuple_reduced_probe.txt"))
    ap.add_argument("--only", default="1,2,3")
    ap.add_argument("--section", default=None, help="run this one section in this process (what the tool starts for every section)")
    ap.add_argument("--train-steps", type=int, default=20000)
    ap.add_argument("--play-max-steps", type=int, default=8192)
    ap.add_argument("--players", default="0,1,2,3,4")
    args = ap.parse_args()
    if args.section is None:
        sys.exit(run_sections(args))
    rows = []

    def say(line=""):
        print(line, flush=True)
        rows.append(line)
        with open(args.out, "w") as f:                      # (kept current: a run that is cut short leaves what it measured)
            f.write("\n".join(rows) + "\n")

    import torch

    import __graft_entry__ as ge
    ge.build()
    import gym2048_amd as g

    say(f"device: {torch.cuda.get_device_name(0)}")
    if args.section in ("1", "2"):
        sets = board_sets(g, torch)
        sets["mid"] = sets["mid"][:N].contiguous()
        nets = {shape: random_net(g, torch, shape) for shape in SHAPES}
        if args.section == "1":
            say(f"late-game set: {len(sets['late'])} distinct boards with 1..4 empty cells, tiled; mid-game set: {len(sets['mid'])} boards, 200 random moves in\n")
            report_constant(say, g, torch, sets, nets)
        else:
            report_schedules(say, g, torch, sets, nets)
    if args.section == "3":
        report_games(say, g, torch, args.train_steps, args.play_max_steps, [int(k) for k in args.players.split(",")])


if __name__ == "__main__":
    main()
