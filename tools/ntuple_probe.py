"""Cost and learning curve of the n-tuple network calls on MI355X; writes profiles/r11_ntuple_probe.txt.

Evaluate: microseconds per launch of g2048_ntuple_evaluate_plain (HIP events, all five outputs) at 2^16 and 2^20 boards
for both default shapes, next to (a) the g2048_afterstates_plain launch on the same boards -- the move work alone, the
floor -- and (b) the torch composition: afterstates, then the 8T indices of every afterstate by tensor ops, torch.take
over them, the sum and the arg-max.  Update: microseconds per launch of g2048_ntuple_update_plain at the same sizes on
boards 200 random steps into their games and on fresh boards (two tiles: the worst same-address contention).
Learning curve: train() from zero weights, mean score of 512 greedy games at a few checkpoints.
ISA: the rows of tools/isa_stats.py for the kernels of the two default shapes (no GPU needed: --isa-only).

  python tools/ntuple_probe.py [--out FILE] [--no-isa] [--no-curve] [--isa-only]
"""
from __future__ import annotations

import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]  # tests/analysis_helpers.py: play()

SIZES = (1 << 16, 1 << 20)
SHAPES = ("4x6", "17x4")
CURVE = {"17x4": dict(boards=1024, lr_shift=10, checkpoints=(0, 2000, 10000, 50000)),
         "4x6": dict(boards=1024, lr_shift=10, checkpoints=(0, 2000, 10000, 50000))}
GAMES = 512


def timed(torch, fn, min_reps=5, budget_ms=400.0):
    """us per call (HIP events), after two warm-up calls."""
    fn(), fn()
    torch.cuda.synchronize()
    reps, spent = 0, 0.0
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    while reps < min_reps or (spent < budget_ms and reps < 200):
        start.record()
        fn()
        end.record()
        end.synchronize()
        spent += start.elapsed_time(end)
        reps += 1
    return spent * 1e3 / reps


def sym_cell_lists(torch, net):
    """int64 [8T, L] cell lists of every (symmetry, tuple) and int64 [8T] table offsets, for the torch composition."""
    import numpy as np
    cells = np.arange(16).reshape(4, 4)
    lists, offs = [], []
    for k in range(4):
        for base in (cells, np.flip(cells, 1)):
            perm = np.rot90(base, k, axes=(1, 0)).reshape(16)
            for t, tup in enumerate(net.tuples):
                lists.append([int(perm[c]) for c in tup])
                offs.append(t * 16 ** net.tuple_len)
    return torch.as_tensor(lists, device="cuda"), torch.as_tensor(offs, device="cuda")


def torch_evaluate(g, torch, net, boards, lists, offs, shifts):
    a = g.afterstates(boards)
    c = a.boards.clamp(max=15).to(torch.int64)                        # [n, 4, 16]
    idx = (c[:, :, lists] << shifts).sum(-1) + offs                    # [n, 4, 8T]
    v = torch.take(net.weights, idx).sum(-1)                           # [n, 4]
    legal = (a.legal.unsqueeze(1) >> torch.arange(4, device="cuda")) & 1
    q = torch.where(legal.bool(), (a.score.to(torch.int64) << net.frac_bits) + v, torch.iinfo(torch.int64).min)
    return q, q.argmax(1)


def isa_rows():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_stats.py"), "ntuple_"], capture_output=True, text=True).stdout
    lines, keep = out.splitlines(), []
    wanted = ("ntuple_eval_kernel<4u, true>", "ntuple_eval_kernel<5u, true>", "ntuple_eval_kernel<4u, false>",
              "ntuple_eval_kernel<5u, false>", "ntuple_values_kernel<4u>", "ntuple_values_kernel<5u>", "ntuple_update_kernel<4u, g2048::NtupleShape, g2048::NtupleBoardItems>",
              "ntuple_update_kernel<5u, g2048::NtupleShape, g2048::NtupleBoardItems>", "ntuple_eval_kernel<8u, true>")
    for i, line in enumerate(lines):
        if any(w in line for w in wanted):
            keep += [line.split("(")[0].replace("void g2048::", "")] + lines[i + 1:i + 3]
    return keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_ntuple_probe.txt"))
    ap.add_argument("--no-isa", action="store_true")
    ap.add_argument("--no-curve", action="store_true")
    ap.add_argument("--isa-only", action="store_true")
    args = ap.parse_args()
    rows = []

    def say(line=""):
        print(line, flush=True)
        rows.append(line)

    if not args.isa_only:
        import torch

        import __graft_entry__ as ge
        ge.build()
        import gym2048_amd as g
        from analysis_helpers import play

        say(f"device: {torch.cuda.get_device_name(0)}")
        eng = g.Batched2048(max(SIZES), seed=7)
        try:
            eng.reset()
            fresh = eng.boards().reshape(-1, 16).clone()
            eng.rollout_random(200)
            played = eng.boards().reshape(-1, 16).clone()
        finally:
            eng.close()
        gen = torch.Generator(device="cuda").manual_seed(1)
        say("\nevaluate: us per launch (all five outputs), boards 200 random steps into their games")
        say("shape       n  gathers/board  ntuple_evaluate  afterstates (floor)  torch composition  composition / kernel  Ggathers/s")
        for shape in SHAPES:
            net = g.NTupleNet(shape)
            net.weights.copy_(torch.randint(-(1 << 20), 1 << 20, net.weights.shape, generator=gen, device="cuda", dtype=torch.int32))
            lists, offs = sym_cell_lists(torch, net)
            shifts = 4 * torch.arange(net.tuple_len, device="cuda")
            for n in SIZES:
                b = played[:n].contiguous()
                out = net.evaluate(b)
                q, act = torch_evaluate(g, torch, net, b, lists, offs, shifts)
                assert torch.equal(q, out.value), "composition != kernel"
                after = g.afterstates(b)
                k_us = timed(torch, lambda: net.evaluate(b, out=out))
                a_us = timed(torch, lambda: g.afterstates(b, out=after))
                t_us = timed(torch, lambda: torch_evaluate(g, torch, net, b, lists, offs, shifts), min_reps=3)
                gathers = 32 * net.n_tuples
                say(f"{shape:5s} {n:7d} {gathers:14d} {k_us:16.1f} {a_us:20.1f} {t_us:18.1f} {t_us / k_us:21.1f} "
                    f"{n * gathers / k_us / 1e3:11.2f}")
        say("\nupdate: us per launch, every step non-zero")
        say("shape       n  atomics/board  played boards  fresh boards  Gatomics/s played  fresh")
        for shape in SHAPES:
            net = g.NTupleNet(shape)
            for n in SIZES:
                delta = torch.randint(1, 1 << 10, (n,), generator=gen, device="cuda", dtype=torch.int64)
                us = [timed(torch, lambda b=b: net.update(b, delta, 0)) for b in (played[:n].contiguous(), fresh[:n].contiguous())]
                atomics = 8 * net.n_tuples
                say(f"{shape:5s} {n:7d} {atomics:14d} {us[0]:14.1f} {us[1]:13.1f} {n * atomics / us[0] / 1e3:18.2f} "
                    f"{n * atomics / us[1] / 1e3:6.2f}")
        if not args.no_curve:
            say(f"\nlearning curve: train() from zero weights, then {GAMES} greedy games to the end (numpy-RNG engine, seed 2048)")
            say("shape  boards  lr_shift  td steps  train s  us/td step  mean score  median     max  mean moves")
            import numpy as np
            for shape, c in CURVE.items():
                net = g.NTupleNet(shape)
                eng = g.Batched2048(c["boards"], seed=11)
                try:
                    eng.reset()
                    done, spent = 0, 0.0
                    for steps in c["checkpoints"]:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        g.train(eng, net, steps - done, c["lr_shift"])
                        torch.cuda.synchronize()
                        spent += time.perf_counter() - t0
                        done = steps
                        act = torch.empty(GAMES, dtype=torch.uint8, device="cuda")
                        pick = g.NTupleEval(None, act, None, None, None)
                        score, illegal, moves, _ = play(g, torch, GAMES, 2048, lambda e, t: e.ntuple_evaluate(net, out=pick).action,
                                                        cap=20000)
                        ok = score >= 0
                        say(f"{shape:5s} {c['boards']:7d} {c['lr_shift']:9d} {steps:9d} {spent:8.1f} "
                            f"{spent * 1e6 / max(1, steps):11.1f} {score[ok].mean():11.1f} {np.median(score[ok]):7.0f} "
                            f"{score[ok].max():7d} {moves / GAMES:11.1f}" + (" (illegal pick!)" if illegal else "")
                            + ("" if ok.all() else f" ({(~ok).sum()} games unfinished at the cap)"))
                finally:
                    eng.close()
    if not args.no_isa:
        say("\nISA (tools/isa_stats.py, gfx950): kernels of the two default shapes (T = 4, 5) and of T = 8")
        for line in isa_rows():
            say(line)
    mode = "a" if args.isa_only and os.path.exists(args.out) else "w"
    with open(args.out, mode) as f:
        f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
