"""Cost and play of tile-downgrading and optimistic initialisation on MI355X; writes
profiles/r30_downgrade_probe.txt.

Translation: us per call of downgrade() (g2048_downgrade_plain: 16 B in, 16 + 1 B out per board) at 2^20 and 2^24 boards of
exponents 0..17, beside a device-to-device copy of the same 16 n bytes timed in the same run, the two alternating; bytes per
second counts what each moves (33 n and 32 n).
Play: us per move of the batch (HIP events around K moves) of ntuple_play as it always was and with downgrade= at min_tile 32
(often at work) and 2^31 (never at work), the three alternating, at 1 024, 65 536 and 2^20 boards for "4x6" and "4x6+4x4";
weights after a short train() run.  The min_tile 2^31 engine is asserted to end on the plain engine's records.
Strength, the protocol of §22: "4x6", frac_bits 10, mean_train at 1 024 boards, lr_shift 6, engine seed 11, 2^28 board-steps,
then play_games at 1 024 boards, one game each, engine seed 2048 -- greedy play with downgrade off and with min_tile 2048, 4096
and 8192 (floor_tile 16); the same four rows for a network trained from fill_value(v), for two v taken from the scores the
zero-initialised network reaches (its mean and its best game).  One seed.

  python tools/downgrade_probe.py [--out FILE] [--no-cost] [--no-play] [--log2-board-steps K]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

PLAIN_SIZES = (1 << 20, 1 << 24)
PLAY_SIZES = (1024, 1 << 16, 1 << 20)
SHAPES = ("4x6", "4x6+4x4")
MIN_TILES = (2048, 4096, 8192)
GAMES = 1024


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30_downgrade_probe.txt"))
    ap.add_argument("--no-cost", action="store_true")
    ap.add_argument("--no-play", action="store_true")
    ap.add_argument("--log2-board-steps", type=int, default=28)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    rows = []

    def say(line=""):
        print(line, flush=True)
        rows.append(line)
        with open(args.out, "w") as f:      # kept current: a run that is cut short leaves what it measured
            f.write("\n".join(rows) + "\n")

    import torch

    import gym2048_amd as g
    from gym2048_amd import _lib
    from ntuple_probe import timed
    _lib.load()

    say(f"device: {torch.cuda.get_device_name(0)}")
    if not args.no_cost:
        say("\ntranslation: downgrade(boards, Downgrade(32, 16)) out of place with `missing`, beside a device-to-device copy of the same")
        say("16 n bytes (Tensor.copy_), us per call (HIP events, three alternating rounds of each); random exponents 0..17")
        say("       n   downgrade us   GB/s (33 n B)     copy us   GB/s (32 n B)   downgrade / copy")
        rule = g.Downgrade(32, 16)
        for n in PLAIN_SIZES:
            boards = torch.randint(0, 18, (n, 16), dtype=torch.uint8, device="cuda")
            out = g.Downgraded(torch.empty_like(boards), torch.empty(n, dtype=torch.uint8, device="cuda"))
            dst = torch.empty_like(boards)
            d_us = c_us = 0.0
            for _ in range(3):
                d_us += timed(torch, lambda: g.downgrade(boards, rule, out=out), budget_ms=100.0) / 3
                c_us += timed(torch, lambda: dst.copy_(boards), budget_ms=100.0) / 3
            at_work = float((out.missing != 0).float().mean())
            say(f"{n:8d} {d_us:14.1f} {33 * n / d_us / 1e3:15.1f} {c_us:11.1f} {32 * n / c_us / 1e3:15.1f} {d_us / c_us:18.2f}"
                f"   (k != 0 on {100 * at_work:.0f} % of the boards)")
            del boards, out, dst
            torch.cuda.empty_cache()

        say("\nplay: us per move of the batch, HIP events around K moves, median (min .. max) of the alternating repetitions after one")
        say("warm-up of each; plain = ntuple_play(net, K); min 32 / min 2^31 = the same with downgrade=Downgrade(32, 16) / (2^31, 16);")
        say("weights after train() of 3000 TD(0) steps on 1024 boards")
        say("shape          n     K   plain us/move            min 32 us/move           min 2^31 us/move         min 32 / plain   min 2^31 / plain")
        for shape in SHAPES:
            net = g.NTupleNet(shape)
            trainer = g.Batched2048(1024, seed=11)
            try:
                trainer.reset()
                g.train(trainer, net, 3000, 10)
            finally:
                trainer.close()
            for n in PLAY_SIZES:
                K = 256 if n >= 1 << 20 else 1024
                engines = [g.Batched2048(n, seed=7) for _ in range(3)]
                rules = (None, g.Downgrade(32, 16), g.Downgrade(1 << 31, 16))
                try:
                    for e, r in zip(engines, rules):
                        e.reset()
                        e.ntuple_play(net, K, downgrade=r)            # warm-up: code objects, allocator
                    ms = [[], [], []]
                    for _ in range(args.reps):
                        for j, (e, r) in enumerate(zip(engines, rules)):
                            ms[j].append(events_ms(torch, lambda: e.ntuple_play(net, K, downgrade=r)))
                    assert torch.equal(engines[0].records(), engines[2].records()), "min_tile 2^31 is not the plain player"
                    us = [[x * 1e3 / K for x in m] for m in ms]
                    med = [statistics.median(u) for u in us]
                    say(f"{shape:8s} {n:8d} {K:5d} " + " ".join(f"{m:9.2f} ({min(u):7.2f} .. {max(u):7.2f})" for m, u in zip(med, us))
                        + f" {med[1] / med[0]:16.3f} {med[2] / med[0]:18.3f}")
                finally:
                    for e in engines:
                        e.close()
            del net
            torch.cuda.empty_cache()

    if not args.no_play:
        total = 1 << args.log2_board_steps
        say(f"\nstrength: \"4x6\", frac_bits 10, mean_train, 1024 boards, lr_shift 6, engine seed 11, {total} board-steps (2^{args.log2_board_steps});")
        say(f"score: play_games, {GAMES} boards, 1 game each, engine seed 2048, greedy play; downgrade = Downgrade(min_tile, 16)")
        say("init value  train s  min_tile  mean score  reach 2048  reach 4096  reach 8192  reach 16384  reach 32768   moves   play s")

        def run(init):
            net = g.NTupleNet("4x6", frac_bits=10, init_value=init)
            mean = g.NTupleMean(net)
            eng = g.Batched2048(1024, seed=11)
            try:
                eng.reset()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                g.mean_train(eng, net, mean, total // 1024, 6)
                torch.cuda.synchronize()
                spent = time.perf_counter() - t0
            finally:
                eng.close()
            first = None
            for tile in (None,) + MIN_TILES:
                player = g.Batched2048(GAMES, seed=2048)
                try:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    rep = g.play_games(player, net, games=1, max_steps=1 << 18, downgrade=None if tile is None else g.Downgrade(tile, 16))
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                finally:
                    player.close()
                first = first or rep
                say(f"{0 if init is None else init:10d} {spent:8.1f} {'off' if tile is None else tile:>9} {rep.mean_score:11.1f} "
                    + " ".join(f"{rep.reach[t]:11.4f}" for t in (2048, 4096, 8192, 16384, 32768)) + f" {rep.moves:9d} {dt:8.2f}"
                    + (f"  ({rep.unfinished} games unfinished)" if rep.unfinished else ""))
            del mean, net
            torch.cuda.empty_cache()
            return first

        base = run(None)
        v_mean, v_best = int(round(base.mean_score)), int(base.scores.max())
        say(f"(the zero-initialised network's games: mean score {v_mean}, best game {v_best}: the two init values below)")
        run(v_mean)
        run(v_best)


if __name__ == "__main__":
    main()
