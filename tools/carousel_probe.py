"""Cost of carousel shaping on MI355X; appends to profiles/r17_carousel_probe.txt.

Times ``td_step`` (HIP events around blocks of steps, after a warm-up that lets episodes end and the pools fill) at 2^20
boards with the 17x4 network in three stages ("has a 64", "has a 256"), without a carousel and with one, alternating the
two in one process, and writes the per-step times of every block, their medians and the ratio; then ``Carousel.step``
alone (its three launches) on the boards the run ended with, without entries and with every live board above stage 0
entering.  ``--no-carousel`` times the plain trainer alone and touches nothing the parent commit lacks: run from a checkout
of the parent commit it gives the parent's figure for the same boards and weights.  Without a GPU the run fails; it does
not fall back.

  python tools/carousel_probe.py [--out FILE] [--no-carousel] [--tag TEXT] [--boards N]
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

WARMUP, BLOCK, REPEATS = 300, 50, 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_carousel_probe.txt"))
    ap.add_argument("--no-carousel", action="store_true", help="time the plain trainer only (also works on the parent commit)")
    ap.add_argument("--tag", default="", help="a label for the header line")
    ap.add_argument("--boards", type=int, default=1 << 20)
    args = ap.parse_args()

    def say(line=""):
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    import torch

    import __graft_entry__ as ge
    ge.build_hip()
    import gym2048_amd as g
    from gym2048_amd import ntuple
    n, shift = args.boards, 6
    thr = (ntuple.stage_mask(64), ntuple.stage_mask(256))
    say(f"\n== {args.tag or 'run'}: {torch.cuda.get_device_name(0)}; td_step, {n} boards, 17x4, stages {[hex(t) for t in thr]}; "
        f"us per step over blocks of {BLOCK} steps after {WARMUP} warm-up steps")

    def setup(with_carousel):
        eng = g.Batched2048(n, seed=7)
        eng.reset()
        net = g.NTupleNet("17x4", stages=thr)
        car = g.Carousel(net, n, capacity=1024, seed=7) if with_carousel else None
        work = ntuple.td_work(eng)
        kw = {"carousel": car} if with_carousel else {}                # the parent's td_step has no such keyword
        step = lambda: ntuple.td_step(eng, net, shift, work, **kw)     # noqa: E731
        for _ in range(WARMUP):
            step()
        torch.cuda.synchronize()
        return eng, net, car, step

    def block(step):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(BLOCK):
            step()
        end.record()
        end.synchronize()
        return start.elapsed_time(end) * 1e3 / BLOCK

    forms = [("plain", setup(False))] + ([] if args.no_carousel else [("carousel", setup(True))])
    times = {name: [] for name, _ in forms}
    for _ in range(REPEATS):                                            # alternating, so that drift hits both alike
        for name, (_, _, _, step) in forms:
            times[name].append(block(step))
    med = {}
    for name, ts in times.items():
        med[name] = sorted(ts)[len(ts) // 2]
        say(f"{name:9s} median {med[name]:9.1f}   blocks " + " ".join(f"{t:9.1f}" for t in ts))
    if "carousel" in med:
        car = forms[1][1][2]
        say(f"ratio carousel / plain (medians): {med['carousel'] / med['plain']:.4f}")
        say(f"carousel after the run: entries per stage {car.count.tolist()}, episodes ended {int(car.episodes.long().sum())}")
        # The two trainers do not play the same boards (restarted boards are further into a game), so the ratio above is of
        # two workloads.  The carousel's own launches, alone, on the boards and the terminated vector the run ended with:
        eng = forms[1][1][0]
        terminated = int(eng.terminated.long().sum())

        def alone(fn, reps=200):
            fn()
            torch.cuda.synchronize()
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(reps):
                fn()
            end.record()
            end.synchronize()
            return start.elapsed_time(end) * 1e3 / reps

        def all_enter():
            car.seen.zero_()
            car.step(eng)

        quiet = [alone(lambda: car.step(eng)) for _ in range(3)]        # a repeated call restarts again, but makes no entry
        above = int((forms[1][1][1].stage(eng.boards()) > 0).sum())
        busy = [alone(all_enter) for _ in range(3)]
        fill = [alone(lambda: car.seen.zero_()) for _ in range(3)]
        say(f"carousel.step alone, us per call (3 x 200 calls): {terminated} boards terminated, no entries: "
            + " ".join(f"{t:7.1f}" for t in quiet))
        say(f"  with seen zeroed before every call, so that every live board above stage 0 ({above} boards are above it) enters: "
            + " ".join(f"{t:7.1f}" for t in busy) + "   (the zeroing alone: " + " ".join(f"{t:5.1f}" for t in fill) + ")")
    for _, (eng, _, _, _) in forms:
        eng.close()


if __name__ == "__main__":
    main()
