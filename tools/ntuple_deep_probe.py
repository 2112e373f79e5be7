"""Cost of the n-tuple deep search (g2048_ntuple_deep_search) on MI355X; writes
profiles/r21_ntuple_deep_probe.txt.  Four measurements, each timed by HIP events around single launches after a warm-up
launch, median (min .. max) of the timed launches:

(1) Depth 3 of the workgroup-per-board kernel, us per launch and network evaluations per second, for the "4x6" and "4x6+4x4"
    networks (random weights: the cost does not depend on them) at 1 024 and 4 096 boards of two sets -- late-game boards
    (1..4 empty cells, the golden trajectories' boards of tests/analysis_helpers.mid_game, tiled to the size) and mid-game
    boards (200 random moves in) -- next to the existing g2048_ntuple_search at depth 2 on the same boards.  Evaluations
    (legal leaf moves of the tree) are counted on a sample by a torch expansion of the tree's shape
    (tools/ntuple_search_probe.py::leaves_per_board): the ratio of the two counts is what the ratio of the times is read against.
(2) THE DECISION NUMBER: the same depth-3 late-game launches through ntuple_search_kernel<3> (one wavefront per board, 16 lanes
    per root direction, each lane walking whole depth-2 trees), from a library built with -DG2048_PROBE_WAVE_DEPTH3
    (--wave-lib FILE; its results are checked equal first).  The workgroup kernel ships only if it is faster here.
(3) Depth 2, new kernel against the existing kernel, 1 024 boards of both sets.  Recorded only.
(4) play_games(player=DeepPlayer(net)) at 256 boards, one game each, on a "4x6" network after a short train() run, next to
    play_games(depth=2) of the same network and seed: wall seconds, moves per second and the PlayReport.  --play-max-steps N
    stops both after N moves per board and reports what is unfinished.

  python tools/ntuple_deep_probe.py --build-wave-lib FILE      # compile the library of (2): needs no GPU, takes minutes
  python tools/ntuple_deep_probe.py [--out FILE] [--wave-lib FILE] [--only 1,2,3,4] [--train-steps N] [--play-max-steps N]
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]

SIZES = (1024, 4096)
SHAPES = ("4x6", "4x6+4x4")
PLAY_BOARDS = 256


def launches_us(torch, fn, budget_ms=1500.0, min_reps=3, max_reps=15):
    """us of single launches of fn() (HIP events), after one warm-up launch: as many as fit the budget, three at the least."""
    fn()
    torch.cuda.synchronize()
    out, spent = [], 0.0
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    while len(out) < min_reps or (spent < budget_ms and len(out) < max_reps):
        start.record()
        fn()
        end.record()
        end.synchronize()
        out.append(start.elapsed_time(end) * 1e3)
        spent += out[-1] / 1e3
    return out


def spread(xs):
    return f"{statistics.median(xs):12.1f} ({min(xs):11.1f} .. {max(xs):11.1f}; {len(xs):2d})"


def overlap(a, b):
    return min(a) <= max(b) and min(b) <= max(a)


def board_sets(g, torch):
    """{"late": uint8 [m, 16] on the device, "mid": [4096, 16]}."""
    import numpy as np
    from analysis_helpers import trajectory_boards
    from ntuple_search_probe import boards_of
    traj = trajectory_boards()
    empties = (traj == 0).sum(1)
    late = traj[(empties >= 1) & (empties <= 4)]
    late = late[np.random.default_rng(21).permutation(len(late))]
    return {"late": torch.as_tensor(np.ascontiguousarray(late)).cuda(), "mid": boards_of(g, torch, max(SIZES), "random")}


def sized(boards, n):
    return boards.repeat(-(-n // len(boards)), 1)[:n].contiguous()


def random_net(g, torch, shape):
    net = g.NTupleNet(shape)
    gen = torch.Generator(device="cuda").manual_seed(21)
    flat = net.weights.view(-1)
    for at in range(0, flat.numel(), 1 << 24):
        part = flat[at:at + (1 << 24)]
        part.copy_(torch.randint(-(1 << 20), 1 << 20, (part.numel(),), generator=gen, device="cuda").to(torch.int32))
    return net


def report_depth3(say, g, torch, sets, nets):
    from ntuple_search_probe import leaves_per_board
    say("(1) depth 3, workgroup per board (g2048_ntuple_deep_search_plain), and the existing depth 2 (g2048_ntuple_search_plain); us per launch,")
    say("    median (min .. max; launches timed); evaluations per board counted on a sample of the same boards")
    say("net       set   boards  empty cells   evals/board d3  evals/board d2   d3 / d2   depth 3 us per launch                          "
        "Gevals/s   depth 2 us per launch                          Gevals/s   time d3 / d2")
    for kind, boards in sets.items():
        sample = boards[:: max(1, len(boards) // (32 if kind == "late" else 8))][:32 if kind == "late" else 8].contiguous()
        e3, e2 = leaves_per_board(g, torch, sample, 3), leaves_per_board(g, torch, sample, 2)
        empties = (boards == 0).sum(1).float()
        for shape, net in nets.items():
            for n in SIZES:
                b = sized(boards, n)
                out = g.NTupleSearch(torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty((n, 4), dtype=torch.int64, device="cuda"))
                d3 = launches_us(torch, lambda: net.deep_search(b, 3, out=out))
                d2 = launches_us(torch, lambda: net.search(b, 2, out=out))
                m3, m2 = statistics.median(d3), statistics.median(d2)
                say(f"{shape:9s} {kind:5s} {n:6d}  {empties.mean().item():5.2f} mean   {e3:14.4e}  {e2:14.4e}  {e3 / e2:8.1f}   {spread(d3)}  "
                    f"{n * e3 / m3 / 1e3:9.2f}   {spread(d2)}  {n * e2 / m2 / 1e3:9.2f}   {m3 / m2:10.1f}")


def bind_wave(path):
    from gym2048_amd import _lib
    lib = C.CDLL(path)
    for name in ("g2048_ntuple_deep_search_plain", "g2048_last_error"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def build_wave_lib(path):
    """The library of (2): the product's sources with build_hip's flags (__graft_entry__.py) and -DG2048_PROBE_WAVE_DEPTH3."""
    import subprocess

    import __graft_entry__ as ge
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra",
           "-mllvm", "-amdgpu-kernarg-preload-count=16", "-DG2048_PROBE_WAVE_DEPTH3", "-o", os.path.abspath(path)]
    subprocess.check_call(cmd + [os.path.join(ge.CSRC, s) for s in ge.HIP_SOURCES], cwd=ge.CSRC)


def report_decision(say, g, torch, sets, nets, wave_path):
    say("\n(2) THE DECISION NUMBER: depth 3 on the late-game set, the workgroup kernel against ntuple_search_kernel<3> (one wavefront per board,")
    say("    the probe-only build -DG2048_PROBE_WAVE_DEPTH3), same boards, same weights, results checked equal; us per launch")
    if not wave_path:
        say("    NOT MEASURED: no probe library was given (--wave-lib)")
        return
    from gym2048_amd import _lib
    wave = bind_wave(wave_path)
    say("net       boards   workgroup per board                                  wavefront per board                                  "
        "wave / workgroup   spreads overlap")
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for shape, net in nets.items():
        for n in SIZES:
            b = sized(sets["late"], n)
            out = g.NTupleSearch(torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty((n, 4), dtype=torch.int64, device="cuda"))
            other = g.NTupleSearch(torch.empty_like(out.action), torch.empty_like(out.value))
            io = _lib.NTupleDeepIO(3, other.action.data_ptr(), other.value.data_ptr(), None)

            def run_wave():
                rc = wave.g2048_ntuple_deep_search_plain(b.data_ptr(), n, net._ref(b.device), C.byref(io), stream())
                assert rc == 0, wave.g2048_last_error()

            net.deep_search(b, 3, out=out)
            run_wave()
            torch.cuda.synchronize()
            assert torch.equal(out.action, other.action) and torch.equal(out.value, other.value), "the two kernels disagree"
            group = launches_us(torch, lambda: net.deep_search(b, 3, out=out))
            wavef = launches_us(torch, run_wave)
            say(f"{shape:9s} {n:6d}   {spread(group)}   {spread(wavef)}   {statistics.median(wavef) / statistics.median(group):16.2f}   "
                f"{'yes' if overlap(group, wavef) else 'no'}")


def report_depth2(say, g, torch, sets, nets):
    say("\n(3) depth 2 at 1 024 boards: the new kernel (deep_search) against the existing kernel (search); recorded only, us per launch")
    say("net       set     deep_search(depth=2)                                 search(depth=2)                                      deep / existing")
    n = 1024
    for kind, boards in sets.items():
        b = sized(boards, n)
        for shape, net in nets.items():
            out = g.NTupleSearch(torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty((n, 4), dtype=torch.int64, device="cuda"))
            ref = net.search(b, 2)
            got = net.deep_search(b, 2)
            assert torch.equal(ref.action, got.action) and torch.equal(ref.value, got.value), "depth 2 differs"
            new = launches_us(torch, lambda: net.deep_search(b, 2, out=out), budget_ms=500.0)
            old = launches_us(torch, lambda: net.search(b, 2, out=out), budget_ms=500.0)
            say(f"{shape:9s} {kind:5s}   {spread(new)}   {spread(old)}   {statistics.median(new) / statistics.median(old):15.2f}")


def report_games(say, g, torch, train_steps, max_steps):
    net = g.NTupleNet("4x6")
    trainer = g.Batched2048(1024, seed=11)
    try:
        trainer.reset()
        g.train(trainer, net, train_steps, 10)
    finally:
        trainer.close()
    say(f"\n(4) play_games at {PLAY_BOARDS} boards, one game each, \"4x6\" after train() of {train_steps} TD(0) steps on 1 024 boards, seed 2048, chunk 32"
        + (f", stopped after {max_steps} moves per board" if max_steps else "") + "; wall seconds of the call (device synchronised)")
    say("player                 seconds   games  unfinished  mean score    moves   moves/s   reach 2048 / 4096 / 8192")
    for name, kw in (("depth=2", dict(depth=2)), ("DeepPlayer(depth=3)", dict(player=g.DeepPlayer(net)))):
        eng = g.Batched2048(PLAY_BOARDS, seed=2048)
        try:
            g.play_games(eng, net, games=1, chunk=4, max_steps=4, **kw)                          # warm-up
            eng.seed(2048)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rep = g.play_games(eng, net, games=1, chunk=32, max_steps=max_steps, **kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        finally:
            eng.close()
        say(f"{name:20s} {dt:9.2f} {rep.games:7d} {rep.unfinished:11d} {rep.mean_score:11.1f} {rep.moves:8d} {rep.moves / dt:9.1f}   "
            f"{rep.reach[2048]:.3f} / {rep.reach[4096]:.3f} / {rep.reach[8192]:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_ntuple_deep_probe.txt"))
    ap.add_argument("--wave-lib", default=None)
    ap.add_argument("--build-wave-lib", default=None, metavar="FILE")
    ap.add_argument("--only", default="1,2,3,4")
    ap.add_argument("--train-steps", type=int, default=3000)
    ap.add_argument("--play-max-steps", type=int, default=None)
    args = ap.parse_args()
    if args.build_wave_lib:
        build_wave_lib(args.build_wave_lib)
        return
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
    only = set(args.only.split(","))
    if only & {"1", "2", "3"}:
        sets = board_sets(g, torch)
        nets = {shape: random_net(g, torch, shape) for shape in SHAPES}
        say(f"late-game set: {len(sets['late'])} distinct boards with 1..4 empty cells, tiled; mid-game set: {len(sets['mid'])} boards, 200 random moves in\n")
        if "1" in only:
            report_depth3(say, g, torch, sets, nets)
        if "2" in only:
            report_decision(say, g, torch, sets, nets, args.wave_lib)
        if "3" in only:
            report_depth2(say, g, torch, sets, nets)
    if "4" in only:
        report_games(say, g, torch, args.train_steps, args.play_max_steps)


if __name__ == "__main__":
    main()
