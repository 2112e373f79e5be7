"""Cost of the n-tuple adaptive search (g2048_ntuple_adaptive_search) on MI355X; the results are kept in
profiles/r23_ntuple_adaptive_probe.txt.  Four measurements; a launch is timed by HIP events after one warm-up launch, 15 launches
per row, median (min .. max).  Board sets and networks are those of tools/ntuple_deep_probe.py: the late-game set (1..4 empty
cells), the mid-game set (200 random moves in), the "4x6" and "4x6+4x4" networks with random weights, 1 024 boards.

(1) The constant schedule 3 against g2048_ntuple_deep_search(depth=3): same boards, same weights, the launches of the two
    interleaved in one process, results checked equal first.  The work is the same: the adaptive kernel's median should lie
    within the deep kernel's own min .. max of that run, or below it.  Also for one and two 4-tuples on the late-game set: the
    adaptive kernel carries the registers of its depth-4 unit, which cost it waves per SIMD at T = 1..6.
(2) The schedules "3-ply-late" and "4-ply-late" on a batch of 512 late-game and 512 mid-game boards (engine form), next to the
    composition of existing calls that gives the bits of "3-ply-late": the masks from the empty cells, ntuple_search(1, active),
    ntuple_search(2, active), ntuple_deep_search(3, active) and the selects.  Recorded only.
(3) Depth 4 (constant schedule 4) on the late-game set: us per launch, evaluations per board (counted on a sample of the same
    boards by the torch expansion of the tree's shape, tools/ntuple_search_probe.py::leaves_per_board) and Gevals/s, next to
    depth 3 on the same boards.
(4) play_games at 256 boards, one game each, "4x6" after a short train() run, seed 2048, chunk 32: DeepPlayer(3),
    AdaptivePlayer("3-ply-late"), AdaptivePlayer("4-ply-late").  One sample on a briefly trained network: it says nothing firm
    about playing strength.

Every section runs in a child process of its own under its own time limit (SECTION_SECONDS); a section that fails or runs out
of time ends the run, and what was measured until then is kept.

  python tools/ntuple_adaptive_probe.py [--out FILE] [--only 1,2,3,4] [--train-steps N] [--play-max-steps N] [--players 0,1,2]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]

from ntuple_deep_probe import PLAY_BOARDS, SHAPES, board_sets, random_net, sized, spread  # noqa: E402

N = 1024
REPS = 15
SMALL = {"1x4": ((0, 1, 2, 3),), "2x4": ((0, 1, 2, 3), (4, 5, 6, 7))}        # T = 1 and 2, for section 1


def interleaved_us(torch, fns, reps=REPS):
    """us of single launches of every fn of ``fns`` (HIP events), one warm-up launch each, then ``reps`` rounds that launch
    them one after the other: [[us of fn 0], [us of fn 1], ...]."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(reps):
        for k, fn in enumerate(fns):
            start.record()
            fn()
            end.record()
            end.synchronize()
            out[k].append(start.elapsed_time(end) * 1e3)
    return out


def adaptive_out(g, torch, n):
    u8 = dict(dtype=torch.uint8, device="cuda")
    return g.NTupleAdaptive(torch.empty(n, **u8), torch.empty((n, 4), dtype=torch.int64, device="cuda"), torch.empty(n, **u8))


def report_constant3(say, g, torch, sets, nets):
    say("(1) constant schedule 3 (g2048_ntuple_adaptive_search_plain) against g2048_ntuple_deep_search_plain(depth=3): 1 024 boards, launches")
    say("    interleaved, results checked equal; us per launch, median (min .. max; launches timed).  \"1x4\" and \"2x4\": one and two 4-tuples,")
    say("    late-game set only, where the adaptive kernel has 4 waves per SIMD against the deep kernel's 6 and 5.")
    say("net       set     adaptive, schedule 3                                 deep_search(depth=3)                                 "
        "adaptive / deep   adaptive median within deep's min .. max, or below")
    small = {name: random_net(g, torch, tuples) for name, tuples in SMALL.items()}
    for kind, boards in sets.items():
        b = sized(boards, N)
        for shape, net in list(nets.items()) + (list(small.items()) if kind == "late" else []):
            out = adaptive_out(g, torch, N)
            ref = g.NTupleSearch(torch.empty_like(out.action), torch.empty_like(out.value))
            net.adaptive_search(b, (3,) * 17, out=out)
            net.deep_search(b, 3, out=ref)
            torch.cuda.synchronize()
            assert torch.equal(out.action, ref.action) and torch.equal(out.value, ref.value), "the two kernels disagree"
            new, old = interleaved_us(torch, [lambda: net.adaptive_search(b, (3,) * 17, out=out), lambda: net.deep_search(b, 3, out=ref)])
            say(f"{shape:9s} {kind:5s}   {spread(new)}   {spread(old)}   {statistics.median(new) / statistics.median(old):15.3f}   "
                f"{'yes' if statistics.median(new) <= max(old) else 'NO'}")


def report_mixed(say, g, torch, sets, nets):
    from gym2048_amd.ntuple import ILLEGAL, SCHEDULES
    say("\n(2) schedules on 512 late-game + 512 mid-game boards (engine form), and the composition of existing calls for \"3-ply-late\" (masks from")
    say("    the empty cells, ntuple_search(1, active), ntuple_search(2, active), ntuple_deep_search(3, active), selects); recorded only, us per call")
    say("net       boards at depth 1 / 2 / 3 (3-ply-late); at 4 (4-ply-late)   adaptive \"3-ply-late\"                                 "
        "composition of existing calls                        adaptive \"4-ply-late\"                                 3-ply adaptive / composition")
    boards = torch.cat([sized(sets["late"], N // 2), sized(sets["mid"], N // 2)]).contiguous()
    empties = (boards == 0).sum(1)
    sched3 = torch.tensor(SCHEDULES["3-ply-late"], device="cuda")
    eng = g.Batched2048(N, seed=23)
    try:
        eng.set_boards(boards.cpu().numpy())
        for shape, net in nets.items():
            out3, out4 = adaptive_out(g, torch, N), adaptive_out(g, torch, N)
            parts = [g.NTupleSearch(torch.empty_like(out3.action), torch.empty_like(out3.value)) for _ in range(3)]
            composed = {}

            def compose():
                depth = sched3[(eng.boards().reshape(-1, 16) == 0).sum(1)]
                masks = [(depth == d).to(torch.int32).view(torch.uint32) for d in (1, 2, 3)]
                eng.ntuple_search(net, 1, out=parts[0], active=masks[0])
                eng.ntuple_search(net, 2, out=parts[1], active=masks[1])
                eng.ntuple_deep_search(net, 3, out=parts[2], active=masks[2])
                action = torch.where(depth == 1, parts[0].action, torch.where(depth == 2, parts[1].action, parts[2].action))
                value = torch.where((depth == 1)[:, None], parts[0].value, torch.where((depth == 2)[:, None], parts[1].value, parts[2].value))
                composed["action"], composed["value"] = action, value

            eng.ntuple_adaptive_search(net, "3-ply-late", out=out3)
            compose()
            torch.cuda.synchronize()
            assert torch.equal(out3.action, composed["action"]) and torch.equal(out3.value, composed["value"]), "the composition disagrees"
            assert bool((out3.value != ILLEGAL).any())
            a3, comp, a4 = interleaved_us(torch, [lambda: eng.ntuple_adaptive_search(net, "3-ply-late", out=out3), compose,
                                                  lambda: eng.ntuple_adaptive_search(net, "4-ply-late", out=out4)])
            counts = [int((sched3[empties] == d).sum()) for d in (1, 2, 3)]
            say(f"{shape:9s} {counts[0]:5d} / {counts[1]:5d} / {counts[2]:5d}; {int((empties <= 1).sum()):5d}                             "
                f"{spread(a3)}   {spread(comp)}   {spread(a4)}   {statistics.median(a3) / statistics.median(comp):10.3f}")
    finally:
        eng.close()


def report_depth4(say, g, torch, sets, nets):
    from ntuple_search_probe import leaves_per_board
    say("\n(3) depth 4 (constant schedule 4) on the late-game set, 1 024 boards, next to depth 3 (constant schedule 3) on the same boards; us per launch;")
    say("    evaluations per board counted on a sample of 8 of the same boards")
    say("net       evals/board d4  evals/board d3   d4 / d3   depth 4 us per launch                          Gevals/s   depth 3 us per launch"
        "                          Gevals/s   time d4 / d3")
    boards = sets["late"]
    sample = boards[:: max(1, len(boards) // 8)][:8].contiguous()
    e4, e3 = leaves_per_board(g, torch, sample, 4), leaves_per_board(g, torch, sample, 3)
    torch.cuda.empty_cache()
    b = sized(boards, N)
    say(f"    (empty cells: {(b == 0).sum(1).float().mean().item():.2f} mean over the batch, {(sample == 0).sum(1).float().mean().item():.2f} over the sample)")
    for shape, net in nets.items():
        out = adaptive_out(g, torch, N)
        d4 = interleaved_us(torch, [lambda: net.adaptive_search(b, (4,) * 17, out=out)])[0]
        d3 = interleaved_us(torch, [lambda: net.adaptive_search(b, (3,) * 17, out=out)])[0]
        m4, m3 = statistics.median(d4), statistics.median(d3)
        say(f"{shape:9s} {e4:14.4e}  {e3:14.4e}  {e4 / e3:8.1f}   {spread(d4)}  {N * e4 / m4 / 1e3:9.2f}   {spread(d3)}  {N * e3 / m3 / 1e3:9.2f}   {m4 / m3:10.1f}")


def report_games(say, g, torch, train_steps, max_steps, players):
    net = g.NTupleNet("4x6")
    trainer = g.Batched2048(1024, seed=11)
    try:
        trainer.reset()
        g.train(trainer, net, train_steps, 10)
    finally:
        trainer.close()
    say(f"\n(4) play_games at {PLAY_BOARDS} boards, one game each, \"4x6\" after train() of {train_steps} TD(0) steps on 1 024 boards, seed 2048, chunk 32"
        + (f", stopped after {max_steps} moves per board" if max_steps else "") + "; wall seconds of the call (device synchronised)")
    say("    One sample on a briefly trained network: it says nothing firm about playing strength.")
    say("player                               seconds   games  unfinished  mean score    moves   moves/s   reach 2048 / 4096 / 8192")
    every = (("DeepPlayer(depth=3)", lambda: g.DeepPlayer(net)), ("AdaptivePlayer(\"3-ply-late\")", lambda: g.AdaptivePlayer(net, "3-ply-late")),
             ("AdaptivePlayer(\"4-ply-late\")", lambda: g.AdaptivePlayer(net, "4-ply-late")))
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


SECTION_SECONDS = {"1": 240, "2": 180, "3": 240, "4": 420}      # the time limit of each section's own process


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_ntuple_adaptive_probe.txt"))
    ap.add_argument("--only", default="1,2,3,4")
    ap.add_argument("--section", default=None, help="run this one section in this process (what the tool starts for every section)")
    ap.add_argument("--train-steps", type=int, default=20000)
    ap.add_argument("--play-max-steps", type=int, default=8192)
    ap.add_argument("--players", default="0,1,2")
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
    only = {args.section}
    if only & {"1", "2", "3"}:
        sets = board_sets(g, torch)
        sets["mid"] = sets["mid"][:N].contiguous()
        nets = {shape: random_net(g, torch, shape) for shape in SHAPES}
        if "1" in only:
            say(f"late-game set: {len(sets['late'])} distinct boards with 1..4 empty cells, tiled; mid-game set: {len(sets['mid'])} boards, 200 random moves in\n")
            report_constant3(say, g, torch, sets, nets)
        if "2" in only:
            report_mixed(say, g, torch, sets, nets)
        if "3" in only:
            report_depth4(say, g, torch, sets, nets)
    if "4" in only:
        report_games(say, g, torch, args.train_steps, args.play_max_steps, [int(k) for k in args.players.split(",")])


if __name__ == "__main__":
    main()
