"""Cost of n-tuple play on MI355X: the fused launch against the per-move composition it replaces; writes
profiles/r19_ntuple_play_probe.txt.

Per move of the whole batch, in microseconds (HIP events around K = 1024 moves, after a warm-up of both forms): (a) the fused
launch, Batched2048.ntuple_play(net, 1024), and (b) the composition, 1024 rounds of ntuple_evaluate with only `action`
requested followed by step(action) -- two launches and several ctypes calls per move.  The two forms are timed in the same
process, alternating, REPS times each; the table gives the median and the spread (min .. max) of both.  Sizes 1024, 65 536 and
2^20 boards, shapes "4x6" and "4x6+4x4", weights after a short train() run, so that the gathers have the locality of a
trained network.  Both engines start from the same seed and play the same games (the fused form is bit-identical, which the
probe asserts on the records).
Wall time: play_games(games=1) at 1024 boards against tests/analysis_helpers.py::play(), which the older probes use, with the
same player -- seconds, moves and microseconds per move.  play() runs a numpy-RNG engine, play_games a spawn-stream one: the
same player, not the same games ("us per played move" = seconds over the moves of running first games, both forms).

  python tools/ntuple_play_probe.py [--out FILE] [--train-steps N] [--reps R]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]  # tests/analysis_helpers.py: play()

SIZES = (1024, 1 << 16, 1 << 20)
SHAPES = ("4x6", "4x6+4x4")
K = 1024
GAMES_BOARDS = 1024


def events_ms(torch, fn):
    """Milliseconds of fn() on the current stream (HIP events; the device is idle before and synchronised after)."""
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_ntuple_play_probe.txt"))
    ap.add_argument("--train-steps", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    rows = []

    def say(line=""):
        print(line, flush=True)
        rows.append(line)

    import torch

    import __graft_entry__ as ge
    ge.build()
    import gym2048_amd as g
    from analysis_helpers import play

    say(f"device: {torch.cuda.get_device_name(0)}")
    say(f"fused = ntuple_play(net, {K}); composed = {K} x (ntuple_evaluate(action only) -> step); us per move of the batch, HIP events,")
    say(f"median (min .. max) of {args.reps} alternating repetitions after one warm-up of each; weights after train() of "
        f"{args.train_steps} TD(0) steps on 1024 boards")
    say("shape          n      fused us/move               composed us/move            composed / fused   fused Mmoves/s")
    nets = {}
    for shape in SHAPES:
        net = nets[shape] = g.NTupleNet(shape)
        trainer = g.Batched2048(1024, seed=11)
        try:
            trainer.reset()
            g.train(trainer, net, args.train_steps, 10)
        finally:
            trainer.close()
        for n in SIZES:
            fused, composed = g.Batched2048(n, seed=7), g.Batched2048(n, seed=7)
            try:
                pick = g.NTupleEval(None, torch.empty(n, dtype=torch.uint8, device="cuda"), None, None, None)

                def run_fused():
                    fused.ntuple_play(net, K)

                def run_composed():
                    for _ in range(K):
                        composed.step(composed.ntuple_evaluate(net, out=pick).action, want_info=False)

                fused.reset(), composed.reset()
                run_fused(), run_composed()                                   # warm-up: code objects, allocator
                torch.cuda.synchronize()
                assert torch.equal(fused.records(), composed.records()), "fused != composed"
                f_ms, c_ms = [], []
                for _ in range(args.reps):
                    f_ms.append(events_ms(torch, run_fused))
                    c_ms.append(events_ms(torch, run_composed))
                assert torch.equal(fused.records(), composed.records()) and fused.clock == composed.clock, "fused != composed"
                f, c = [x * 1e3 / K for x in f_ms], [x * 1e3 / K for x in c_ms]
                fm, cm = statistics.median(f), statistics.median(c)
                say(f"{shape:8s} {n:8d}   {fm:9.2f} ({min(f):8.2f} .. {max(f):8.2f})   {cm:9.2f} ({min(c):8.2f} .. {max(c):8.2f})   "
                    f"{cm / fm:16.2f}   {n / fm:14.1f}")
            finally:
                fused.close(), composed.close()

    say(f"\nwall time of every board's first game, {GAMES_BOARDS} boards, the same player: play_games(games=1) (spawn-stream engine, one host")
    say("read per 1024 moves) against tests/analysis_helpers.py::play() (numpy-RNG engine, host reads after every move); not the same games")
    say("shape     form         seconds   games  mean score  moves played  us per played move")
    for shape in SHAPES:
        net = nets[shape]
        eng = g.Batched2048(GAMES_BOARDS, seed=2048)
        try:
            g.play_games(eng, net, games=1, max_steps=K)                      # warm-up
            eng.seed(2048)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rep = g.play_games(eng, net, games=1)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            say(f"{shape:8s}  play_games  {dt:8.3f} {rep.games:7d} {rep.mean_score:11.1f} {rep.moves:13d} {dt * 1e6 / max(1, rep.moves):19.3f}"
                + ("" if rep.unfinished == 0 else f" ({rep.unfinished} unfinished)"))
        finally:
            eng.close()
        pick = g.NTupleEval(None, torch.empty(GAMES_BOARDS, dtype=torch.uint8, device="cuda"), None, None, None)
        score, illegal, moves, dt = play(g, torch, GAMES_BOARDS, 2048, lambda e, t: e.ntuple_evaluate(net, out=pick).action, cap=100000)
        ok = score >= 0
        say(f"{shape:8s}  play()      {dt:8.3f} {int(ok.sum()):7d} {score[ok].mean():11.1f} {moves:13d} {dt * 1e6 / max(1, moves):19.3f}"
            + (" (illegal pick!)" if illegal else ""))
    with open(args.out, "w") as f:
        f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
