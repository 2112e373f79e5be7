"""Cost and learning of the midpoint restart on MI355X; writes profiles/r29_restart_probe.txt.

Time (HIP events around a train of back-to-back calls, nothing else on the device; the per-call figure of a train is its time
over its calls; median (min .. max) over the trains):
  restart   Restart.step(engine): one g2048_restart_step launch, TRAINS trains of CALLS calls; the engine stands still, so every
            call sees the same records and terminated; pos moves on, so one call in `stride` stores a snapshot
  td_step   td_step(engine, net) at the same size, the forward TD(0) step the restart step sits in: trains of TD_CALLS steps
at 1 024, 65 536 and 2^20 boards, "4x6", stride 16, capacity 256, min_span 64.
  play_log / play_log_restart   Batched2048.ntuple_play_log(net, log) without and with restart=, us per move of the batch,
            M = 16, interleaved, at 1 024 and 65 536 boards; the weights are only read
Learning: "4x6", frac_bits 10, zero weights, engine seed 11, 2^28 board-steps at 1 024 boards, scored by play_games at 1 024
boards, one game each (engine seed 2048): train() and backward_train(tc=, M = 16), each without and with
restart=Restart(stride=16, capacity=256, min_span=64).  One seed: a direction.

  python tools/restart_probe.py [--out FILE] [--no-time] [--no-learn] [--log2-board-steps K]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

SIZES = (1 << 10, 1 << 16, 1 << 20)
LOG_SIZES = (1 << 10, 1 << 16)
TRAINS, CALLS, TD_CALLS = 20, 100, 20
DEPTH, GAMES = 16, 1024
RULE = dict(stride=16, capacity=256, min_span=64)
LEARN = (("train", 12), ("backward-tc", 10))                     # the best lr_shift of each at 1 024 boards


def events_ms(torch, fn):
    """Milliseconds of fn() on the current stream (HIP events; the device is idle before and synchronised after)."""
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


def spread(v):
    return f"{statistics.median(v):8.2f} ({min(v):7.2f} .. {max(v):7.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_restart_probe.txt"))
    ap.add_argument("--no-time", action="store_true")
    ap.add_argument("--no-learn", action="store_true")
    ap.add_argument("--append", action="store_true", help="keep what --out already holds")
    ap.add_argument("--log2-board-steps", type=int, default=28)
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
        net = g.NTupleNet("4x6")
        warm = g.Batched2048(1024, seed=11)
        try:
            warm.reset()
            g.train(warm, net, 3000, 10)                                  # weights with the locality of a trained network
        finally:
            warm.close()
        start = net.weights.clone()
        say(f"\nrestart step: us per call, median (min .. max) of {TRAINS} trains of {CALLS} back-to-back Restart.step(engine) calls "
            f"({TRAINS * CALLS} calls);")
        say(f"td_step: us per step, {TRAINS} trains of {TD_CALLS} td_step(engine, net) calls, \"4x6\", weights restored before every train;")
        say(f"stride {RULE['stride']}, capacity {RULE['capacity']}, min_span {RULE['min_span']}; bytes/board = 16 capacity + 12 of restart state")
        say("       n   restart step us                  td_step us                     restart / td_step   terminated boards")
        for n in SIZES:
            eng = g.Batched2048(n, seed=7)
            try:
                eng.reset()
                r = g.Restart(n, **RULE)
                g.train(eng, net, 300, 10, restart=r)                     # some episodes under way, pos off the stride grid
                work = g.td_work(eng)
                step_us, td_us = [], []
                r.step(eng)
                for _ in range(TRAINS):
                    step_us.append(events_ms(torch, lambda: [r.step(eng) for _ in range(CALLS)]) * 1e3 / CALLS)
                    net.weights.copy_(start)
                    td_us.append(events_ms(torch, lambda: [g.td_step(eng, net, 10, work) for _ in range(TD_CALLS)]) * 1e3 / TD_CALLS)
                say(f"{n:8d}  {spread(step_us)}  {spread(td_us)}  {statistics.median(step_us) / statistics.median(td_us):17.3f}"
                    f"  {int(eng.terminated.sum()):8d}")
                del r, work
            finally:
                eng.close()
            torch.cuda.empty_cache()
        say(f"\nplay_log against play_log_restart: us per move of the batch, M = {DEPTH}, \"4x6\", median (min .. max) of {TRAINS} interleaved")
        say("windows of 64 calls (16 at 65 536 boards) each; the two forms run on one engine, which plays on from window to window")
        say("       n   play_log us                      play_log_restart us            restart / plain")
        for n in LOG_SIZES:
            eng = g.Batched2048(n, seed=7)
            try:
                eng.reset()
                r, log = g.Restart(n, **RULE), g.NTupleLog(n, depth=DEPTH)
                calls = 64 if n <= 1 << 10 else 16
                plain = lambda: [eng.ntuple_play_log(net, log) for _ in range(calls)]                  # noqa: E731
                again = lambda: [eng.ntuple_play_log(net, log, restart=r) for _ in range(calls)]       # noqa: E731
                plain(), again()
                us = {"plain": [], "again": []}
                for _ in range(TRAINS):
                    us["plain"].append(events_ms(torch, plain) * 1e3 / (calls * DEPTH))
                    us["again"].append(events_ms(torch, again) * 1e3 / (calls * DEPTH))
                say(f"{n:8d}  {spread(us['plain'])}  {spread(us['again'])}  {statistics.median(us['again']) / statistics.median(us['plain']):15.3f}")
                del r, log
            finally:
                eng.close()
            torch.cuda.empty_cache()
    if not args.no_learn:
        total, n = 1 << args.log2_board_steps, 1024
        say(f"\nlearning: \"4x6\", frac_bits 10, zero weights, engine seed 11, {n} boards, {total} board-steps per run (2^{args.log2_board_steps});")
        say(f"score: play_games, {GAMES} boards, 1 game each, engine seed 2048; backward-tc = backward_train(tc=), M = {DEPTH};")
        say(f"restart = Restart(stride={RULE['stride']}, capacity={RULE['capacity']}, min_span={RULE['min_span']})")
        say("learner      restart  lr_shift     steps  train s  episode ends  mean score  reach 2048  reach 4096  reach 8192")
        for kind, shift in LEARN:
            for with_restart in (False, True):
                net = g.NTupleNet("4x6", frac_bits=10)
                eng = g.Batched2048(n, seed=11)
                try:
                    eng.reset()
                    r = g.Restart(n, **RULE) if with_restart else None
                    steps = total // n
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    if kind == "train":
                        g.train(eng, net, steps, shift, restart=r)
                    else:
                        g.backward_train(eng, net, g.NTupleLog(n, depth=DEPTH), steps // DEPTH, shift, tc=g.NTupleTC(net), restart=r)
                    torch.cuda.synchronize()
                    spent = time.perf_counter() - t0
                    episodes = eng.episode_stats()["episodes"]
                finally:
                    eng.close()
                player = g.Batched2048(GAMES, seed=2048)
                try:
                    rep = g.play_games(player, net, games=1, max_steps=1 << 17)
                finally:
                    player.close()
                say(f"{kind:11s} {'yes' if with_restart else 'no':>8s} {shift:9d} {steps:9d} {spent:8.1f} "
                    f"{episodes:13d} {rep.mean_score:11.1f} {rep.reach[2048]:11.4f} "
                    f"{rep.reach[4096]:11.4f} {rep.reach.get(8192, 0.0):11.4f}" + (f"  ({rep.unfinished} games unfinished)" if rep.unfinished else ""))
                del net, r
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
