"""Cost and learning of backward learning over logged segments on MI355X; writes
profiles/r28_ntuple_log_probe.txt.

Time: us per move of the whole batch (HIP events), the forms interleaved REPS times in one process, median (min .. max):
  round     backward_train, TD: ONE g2048_ntuple_log_train call of R rounds of M moves, R * M about STEPS; 1 + 2M launches a round
  play      Batched2048.ntuple_play_log alone, one launch per M moves
  delta     NTupleNet.log_delta alone, a Python loop over the M slots
  update    NTupleNet.update of a slot alone, a Python loop over the M slots
  composed  train(fused=False), the forward TD(0) learner: eight launches per step
  fused     train(fused=True): one g2048_ntuple_td_train call, two launches per step
at 1 024, 16 384, 65 536 and 2^20 boards, M = 4, 16 and 64, for "4x6" and "4x6+4x4"; weights after a short train() run, so that
the gathers have the locality of a trained network, restored before every timed window; a window is MOVES[n] moves, 0.1 s or
more.  play, delta and update are library calls from Python, one per launch: at
small batches they include what the C trainer saves, so their sum is above `round` there.  Beside them the delta launch against
the two g2048_ntuple_values_plain launches that compute the same two values.
Learning: "4x6", frac_bits 10, zero weights, engine seed 11, every run the same number of board-steps; train(), tdl_train(H = 4,
lambda = 0.5) and backward_train(M = 16), TD and TC, under the lr_shift candidates of tools/ntuple_mean_probe.py at 1 024 and
65 536 boards.  Each net is scored by play_games at 1 024 boards, one game each (engine seed 2048).  One seed: a direction.

  python tools/ntuple_log_probe.py [--out FILE] [--no-time] [--no-learn] [--log2-board-steps K] [--reps R]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

SIZES = (1 << 10, 1 << 14, 1 << 16, 1 << 20)
SHAPES = ("4x6", "4x6+4x4")
DEPTHS = (4, 16, 64)
LR_SHIFT = 10
MOVES = {1 << 10: 1536, 1 << 14: 1536, 1 << 16: 384, 1 << 20: 64}      # per timed window: 0.1 s or more at every size
LEARN_SIZES = {1 << 10: (8, 10, 12), 1 << 16: (12, 14, 16, 18)}     # the candidates of tools/ntuple_mean_probe.py
LEARN_DEPTH, GAMES = 16, 1024


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_ntuple_log_probe.txt"))
    ap.add_argument("--no-time", action="store_true")
    ap.add_argument("--no-learn", action="store_true")
    ap.add_argument("--append", action="store_true", help="keep what --out already holds")
    ap.add_argument("--log2-board-steps", type=int, default=28)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    rows = open(args.out).read().splitlines() if args.append and os.path.exists(args.out) else []

    def say(line=""):
        print(line, flush=True)
        rows.append(line)
        with open(args.out, "w") as f:      # kept current: a run that is cut short leaves what it measured
            f.write("\n".join(rows) + "\n")

    import torch

    import gym2048_amd as g
    from gym2048_amd import _lib
    _lib.load()

    say(f"device: {torch.cuda.get_device_name(0)}")
    if not args.no_time:
        say(f"\ntime: us per move of the batch, HIP events, median (min .. max) of {args.reps} interleaved repetitions; lr_shift {LR_SHIFT};")
        say("weights after train() of 3000 TD(0) steps on 1024 boards, restored before every timed window; a window is "
            + ", ".join(f"{v} moves at {k}" for k, v in MOVES.items()) + " boards;")
        say("the engine is one per size and plays on from window to window, so the boards of a row are not those of another row")
        say("round = one g2048_ntuple_log_train call (TD); play / delta / update = the three kinds of launch alone, from Python;")
        say("composed = train(fused=False); fused = train(fused=True)")
        say("shape          n   M    round (    min ..     max)     play    delta   update  composed    fused  composed/round")
        layout = []
        for shape in SHAPES:
            net = g.NTupleNet(shape)
            warm = g.Batched2048(1024, seed=11)
            try:
                warm.reset()
                g.train(warm, net, 3000, LR_SHIFT)
            finally:
                warm.close()
            start = net.weights.clone()
            for n in SIZES:
                steps = MOVES[n]
                eng = g.Batched2048(n, seed=7)
                try:
                    eng.reset()
                    delta = torch.zeros(n, dtype=torch.int64, device=eng.device)
                    for M in DEPTHS:
                        R = max(1, steps // M)
                        log = g.NTupleLog(n, depth=M)
                        forms = {
                            "round": lambda: eng.ntuple_log_train(net, log, R, LR_SHIFT, delta),
                            "play": lambda: [eng.ntuple_play_log(net, log) for _ in range(R)],
                            "delta": lambda: [net.log_delta(log, m, out=delta) for _ in range(R) for m in range(M - 1, -1, -1)],
                            "update": lambda: [net.update(log.slot(m), delta, LR_SHIFT) for _ in range(R) for m in range(M - 1, -1, -1)],
                            "composed": lambda: g.train(eng, net, R * M, LR_SHIFT),
                            "fused": lambda: g.train(eng, net, R * M, LR_SHIFT, fused=True),
                        }
                        for fn in forms.values():
                            fn()                                              # warm-up: code objects, allocator
                        us = {name: [] for name in forms}
                        for _ in range(args.reps):
                            for name, fn in forms.items():
                                net.weights.copy_(start)                      # every window reads and moves the same weights
                                us[name].append(events_ms(torch, fn) * 1e3 / (R * M))
                        med = {name: statistics.median(v) for name, v in us.items()}
                        say(f"{shape:8s} {n:8d} {M:3d} {med['round']:8.2f} ({min(us['round']):7.2f} .. {max(us['round']):7.2f}) {med['play']:8.2f} "
                            f"{med['delta']:8.2f} {med['update']:8.2f} {med['composed']:9.2f} {med['fused']:8.2f} {med['composed'] / med['round']:15.2f}")
                        if M == 16:                                           # the delta launch against two values launches
                            one = [events_ms(torch, lambda: [net.log_delta(log, m, out=delta) for m in range(M)]) * 1e3 / M for _ in range(args.reps)]
                            two = [events_ms(torch, lambda: [(net.values(log.slot(m), out=delta), net.values(log.slot(m + 1), out=delta))
                                                             for m in range(M)]) * 1e3 / M for _ in range(args.reps)]
                            layout.append(f"{shape:8s} {n:8d} {statistics.median(one):10.2f} {statistics.median(two):18.2f}")
                        del log
                        torch.cuda.empty_cache()
                finally:
                    eng.close()
            del net, start
            torch.cuda.empty_cache()
        say("\nthe delta launch (one board per lane, up to two evaluations) against two g2048_ntuple_values_plain launches on the same two")
        say(f"slots, us per slot, median of {args.reps}, M = 16:")
        say("shape          n  log_delta  2 x values_plain")
        for line in layout:
            say(line)
    if not args.no_learn:
        total = 1 << args.log2_board_steps
        say(f"\nlearning: \"4x6\", frac_bits 10, zero weights, engine seed 11, {total} board-steps per run (2^{args.log2_board_steps});")
        say(f"score: play_games, {GAMES} boards, 1 game each, engine seed 2048; backward = backward_train, M = {LEARN_DEPTH}; tdl = tdl_train, H = 4, lambda = 0.5")
        say("learner      boards  lr_shift     steps  train s  mean score  reach 2048  reach 4096")

        def run(kind, n, shift):
            net = g.NTupleNet("4x6", frac_bits=10)
            tc = g.NTupleTC(net) if kind == "backward-tc" else None
            eng = g.Batched2048(n, seed=11)
            try:
                eng.reset()
                steps = total // n
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if kind == "train":
                    g.train(eng, net, steps, shift)
                elif kind == "tdl":
                    g.tdl_train(eng, net, g.NTupleTrace(n, depth=4, lam=0.5), steps, shift)
                else:
                    g.backward_train(eng, net, g.NTupleLog(n, depth=LEARN_DEPTH), steps // LEARN_DEPTH, shift, tc=tc)
                torch.cuda.synchronize()
                spent = time.perf_counter() - t0
            finally:
                eng.close()
            player = g.Batched2048(GAMES, seed=2048)
            try:
                rep = g.play_games(player, net, games=1, max_steps=1 << 17)
            finally:
                player.close()
            say(f"{kind:11s} {n:7d} {shift:9d} {steps:9d} {spent:8.1f} {rep.mean_score:11.1f} {rep.reach[2048]:11.4f} {rep.reach[4096]:11.4f}"
                + (f"  ({rep.unfinished} games unfinished)" if rep.unfinished else ""))
            del tc, net
            torch.cuda.empty_cache()

        for n, shifts in LEARN_SIZES.items():
            for kind in ("train", "tdl", "backward-td", "backward-tc"):
                for s in shifts:
                    run(kind, n, s)


if __name__ == "__main__":
    main()
