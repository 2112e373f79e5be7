"""Cost of the fused n-tuple TD step on MI355X against the composition it replaces; writes profiles/r25_ntuple_td_probe.txt.

Per TD(0) step of the whole batch, in microseconds (HIP events around STEPS steps, after a warm-up of WARMUP steps of every
form), three forms in one process:
  composed   train(fused=False): evaluate, step, evaluate, four element-wise torch launches, update -- eight launches and
             the Python between them; the parent's path, unchanged
  trainer    train(fused=True): ONE g2048_ntuple_td_train call, two launches per step, no Python between the steps
  loop       a Python loop of td_step(fused=True): two launches and two library calls per step
The three forms are timed interleaved, REPS times each; the table gives the median and the spread (min .. max) of each, and
boards * steps / s of the median.  Sizes 1 024, 16 384, 65 536 and 2^20 boards, shapes "4x6" and "4x6+4x4", weights after a
short train() run, so that the gathers have the locality of a trained network; each form trains a copy of its own.  All three
engines start from the same seed; the forms are bit-identical, which the probe asserts on the records and the weights.

  python tools/ntuple_td_probe.py [--out FILE] [--train-steps N] [--reps R]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

SIZES = (1024, 1 << 14, 1 << 16, 1 << 20)
SHAPES = ("4x6", "4x6+4x4")
STEPS, WARMUP, LR_SHIFT = 200, 20, 10
FORMS = ("composed", "trainer", "loop")


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_ntuple_td_probe.txt"))
    ap.add_argument("--train-steps", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    rows = []

    def say(line=""):
        print(line, flush=True)
        rows.append(line)

    import torch

    import __graft_entry__ as ge
    ge.build()
    import gym2048_amd as g
    from gym2048_amd import ntuple

    say(f"device: {torch.cuda.get_device_name(0)}")
    say(f"us per TD(0) step of the batch, HIP events around {STEPS} steps after a warm-up of {WARMUP}; median (min .. max) of {args.reps}")
    say(f"interleaved repetitions; lr_shift {LR_SHIFT}; weights after train() of {args.train_steps} TD(0) steps on 1024 boards")
    say("composed = train(fused=False), 8 launches per step; trainer = train(fused=True), one g2048_ntuple_td_train call; "
        "loop = Python loop of td_step(fused=True)")
    say("shape          n  form       us/step   (     min ..      max)   boards*steps/s   composed/this")
    verdicts = []
    for shape in SHAPES:
        trained = g.NTupleNet(shape)
        trainer = g.Batched2048(1024, seed=11)
        try:
            trainer.reset()
            g.train(trainer, trained, args.train_steps, LR_SHIFT)
        finally:
            trainer.close()
        for n in SIZES:
            engines = {form: g.Batched2048(n, seed=7) for form in FORMS}
            nets = {}
            for form in FORMS:
                nets[form] = g.NTupleNet(shape)
                nets[form].weights.copy_(trained.weights)
            try:
                work = ntuple.td_work(engines["loop"])

                def loop(k):
                    for _ in range(k):
                        ntuple.td_step(engines["loop"], nets["loop"], LR_SHIFT, work, fused=True)

                run = {"composed": lambda k: g.train(engines["composed"], nets["composed"], k, LR_SHIFT),
                       "trainer": lambda k: g.train(engines["trainer"], nets["trainer"], k, LR_SHIFT, fused=True),
                       "loop": loop}
                for form in FORMS:
                    engines[form].reset()
                    run[form](WARMUP)                                         # warm-up: code objects, allocator
                ms = {form: [] for form in FORMS}
                for _ in range(args.reps):
                    for form in FORMS:
                        ms[form].append(events_ms(torch, lambda: run[form](STEPS)))
                for form in FORMS[1:]:
                    assert torch.equal(engines[form].records(), engines["composed"].records()), f"{form} != composed: records"
                    assert engines[form].clock == engines["composed"].clock, f"{form} != composed: clock"
                    assert torch.equal(nets[form].weights, nets["composed"].weights), f"{form} != composed: weights"
                us = {form: [x * 1e3 / STEPS for x in ms[form]] for form in FORMS}
                med = {form: statistics.median(us[form]) for form in FORMS}
                for form in FORMS:
                    say(f"{shape:8s} {n:8d}  {form:8s} {med[form]:9.2f}   ({min(us[form]):8.2f} .. {max(us[form]):8.2f})   "
                        f"{n / med[form] * 1e6:14.3e}   {med['composed'] / med[form]:13.2f}")
                verdicts.append((shape, n, med["trainer"] < min(us["composed"]), med["loop"] < min(us["composed"])))
            finally:
                for e in engines.values():
                    e.close()
    say()
    say("fused median below the composed form's minimum of the same run (trainer, loop):")
    for shape, n, trainer_wins, loop_wins in verdicts:
        say(f"{shape:8s} {n:8d}  {'yes' if trainer_wins else 'NO':4s} {'yes' if loop_wins else 'NO'}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
