"""Cost of the budgeted play step and of the masked search on MI355X; writes
profiles/r20_play_step_probe.txt.  Three measurements:

(1) Wall time of play_games(games=1) at 1024 boards for depth 1 and 2 on the "4x6" network after a short train() run, with the
    search masked by games_left (active=left, what play_games does) and with the skip disabled (--skip off: the probe hands
    play_games an engine whose ntuple_search drops the mask).  Moves per game, and network evaluations per second: the
    evaluations (legal leaf moves of the searched trees, tools/ntuple_search_probe.py::leaves_per_board) are counted in an
    untimed replay of the same games on a sample -- every COUNT_EVERY-th move, at most COUNT_BOARDS of the boards that
    still play -- and scaled up; the unmasked run searches all n boards at every move, resting ones on their fresh board.
(2) Microseconds per launch of the UNCHANGED ntuple_search call at depth 1 and 2 (2^12 and 2^16 boards) on this library and
    on a library built from the parent commit (--parent-lib FILE; both through ctypes in this process, the same boards and
    weights), at least five alternating repetitions each, HIP events: both medians, the parent's own min .. max spread, and
    whether the new figure lies inside it.  Without --parent-lib the file says that this was not measured.
(3) Microseconds per play_step against step(want_info=False) at 2^12, 2^16 and 2^20 boards.  Recorded only.

  python tools/play_step_probe.py [--out FILE] [--train-steps N] [--reps R] [--parent-lib FILE] [--skip on|off|both] [--only 1,2,3]
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

BOARDS = 1024
COUNT_EVERY, COUNT_BOARDS = 16, 128
SEARCH_SIZES = (1 << 12, 1 << 16)
STEP_SIZES = (1 << 12, 1 << 16, 1 << 20)
LAUNCHES = 20           # launches per timed repetition of (2); (3) times 256 steps


def events_ms(torch, fn):
    """Milliseconds of fn() on the current stream (HIP events; the device is idle before and synchronised after)."""
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


def spread(xs):
    return f"{statistics.median(xs):9.2f} ({min(xs):8.2f} .. {max(xs):8.2f})"


def count_evaluations(g, torch, net, depth, seed, masked):
    """An untimed replay of play_games(games=1, depth=depth) from ``seed``: (moves played, estimated network evaluations of all
    searches).  Sampled: see the module docstring."""
    from ntuple_search_probe import leaves_per_board
    eng = g.Batched2048(BOARDS, seed=seed)
    try:
        eng.reset()
        left = torch.ones(BOARDS, dtype=torch.int32, device=eng.device).view(torch.uint32)
        act = torch.empty(BOARDS, dtype=torch.uint8, device=eng.device)
        fresh_leaves, total, per_board, move = None, 0.0, 0.0, 0
        while True:
            playing = left.view(torch.int32) != 0
            n_playing = int(playing.sum())
            if n_playing == 0:
                break
            if move % COUNT_EVERY == 0:
                boards = eng.boards().reshape(-1, 16)
                sample = boards[playing][:COUNT_BOARDS].contiguous()
                per_board = leaves_per_board(g, torch, sample, depth)
                if fresh_leaves is None:                             # every board is a fresh two-tile board at move 0
                    fresh_leaves = per_board
            total += n_playing * per_board + (0 if masked else (BOARDS - n_playing) * fresh_leaves)
            eng.ntuple_search(net, depth, out=g.NTupleSearch(act, None), active=left)
            eng.play_step(act, games_left=left)
            move += 1
        return move, total
    finally:
        eng.close()


def report_games(say, g, torch, net, skips):
    say(f"(1) play_games(games=1, depth=d) at {BOARDS} boards, \"4x6\"; wall seconds of the call (perf_counter around it, device synchronised),")
    say("    one warm-up call before; evaluations = legal leaf moves of the searched trees, sampled in an untimed replay")
    say("depth  skip   seconds   games  mean score   moves  moves/game  search launches   evaluations  Mevaluations/s")
    seconds = {}
    for depth in (1, 2):
        for skip in skips:
            eng = g.Batched2048(BOARDS, seed=2048)
            try:
                if skip == "off":
                    search = eng.ntuple_search
                    eng.ntuple_search = lambda net, depth=1, out=None, active=None: search(net, depth, out=out)
                g.play_games(eng, net, games=1, chunk=64, max_steps=64, depth=depth)          # warm-up
                eng.seed(2048)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rep = g.play_games(eng, net, games=1, chunk=256, depth=depth)
                torch.cuda.synchronize()
                dt = seconds[depth, skip] = time.perf_counter() - t0
            finally:
                eng.close()
            launches, evals = count_evaluations(g, torch, net, depth, 2048, skip == "on")
            say(f"{depth:5d}  {skip:4s} {dt:9.3f} {rep.games:7d} {rep.mean_score:11.1f} {rep.moves:7d} {rep.moves / max(1, rep.games):11.1f} "
                f"{launches:16d} {evals:13.3e} {evals / dt / 1e6:15.1f}" + ("" if rep.unfinished == 0 else f" ({rep.unfinished} unfinished)"))
        if (depth, "on") in seconds and (depth, "off") in seconds:
            say(f"       depth {depth}: unmasked / masked wall time = {seconds[depth, 'off'] / seconds[depth, 'on']:.2f} (recorded; no threshold)")


def bind(path):
    """A second copy of the library (the parent commit's) behind ctypes, with the prototypes of the symbols (2) uses."""
    from gym2048_amd import _lib
    lib = C.CDLL(path)
    for name in ("g2048_create", "g2048_destroy", "g2048_reset", "g2048_rollout_random", "g2048_ntuple_search", "g2048_last_error"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def report_search(say, g, torch, net, parent_path, reps):
    say("\n(2) the unchanged g2048_ntuple_search (action and value), us per launch, HIP events around "
        f"{LAUNCHES} launches, median (min .. max) of {reps} alternating repetitions")
    if not parent_path:
        say("    NOT MEASURED: no library of the parent commit was given (--parent-lib)")
        return
    from gym2048_amd import _lib
    libs = {"parent": bind(parent_path), "this": _lib.load()}
    say("depth    boards   parent us/launch              this commit us/launch         inside the parent's spread")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for depth in (1, 2):
        for n in SEARCH_SIZES:
            action = torch.empty(n, dtype=torch.uint8, device="cuda")
            value = torch.empty((n, 4), dtype=torch.int64, device="cuda")
            io = _lib.NTupleSearchIO(depth, action.data_ptr(), value.data_ptr())
            engines, got = {}, {}
            try:
                for name, lib in libs.items():
                    h = C.c_void_p()
                    assert lib.g2048_create(n, 0, 7, 0, C.byref(h)) == 0, lib.g2048_last_error()
                    engines[name] = h
                    assert lib.g2048_reset(h, 1, 0, None, stream) == 0 and lib.g2048_rollout_random(h, 200, stream) == 0

                def run(name):
                    for _ in range(LAUNCHES):
                        libs[name].g2048_ntuple_search(engines[name], net._ref(action.device), C.byref(io), stream)

                for name in libs:
                    run(name)                                        # warm-up; and both must give the same bits
                    torch.cuda.synchronize()
                    got[name] = (action.clone(), value.clone())
                assert all(torch.equal(a, b) for a, b in zip(got["parent"], got["this"])), "the two libraries disagree"
                us = {name: [] for name in libs}
                for _ in range(reps):
                    for name in libs:
                        us[name].append(events_ms(torch, lambda: run(name)) * 1e3 / LAUNCHES)
                inside = min(us["parent"]) <= statistics.median(us["this"]) <= max(us["parent"])
                say(f"{depth:5d} {n:9d}   {spread(us['parent'])}   {spread(us['this'])}   {'yes' if inside else 'NO'}")
            finally:
                for name, h in engines.items():
                    libs[name].g2048_destroy(h)


def report_step(say, g, torch, reps):
    k = 256
    say(f"\n(3) play_step(actions) against step(actions, want_info=False): us per step, HIP events around {k} steps of uint8 actions,")
    say(f"    median (min .. max) of {reps} alternating repetitions; recorded only")
    say("   boards   play_step us                  step us                       play_step / step")
    for n in STEP_SIZES:
        a, b = g.Batched2048(n, seed=7), g.Batched2048(n, seed=7)
        try:
            a.reset(), b.reset()
            acts = a.random_actions(k)

            def run_play():
                for j in range(k):
                    a.play_step(acts[j])

            def run_step():
                for j in range(k):
                    b.step(acts[j], want_info=False)

            run_play(), run_step()
            torch.cuda.synchronize()
            assert torch.equal(a.records(), b.records()), "play_step != step"
            p, s = [], []
            for _ in range(reps):
                p.append(events_ms(torch, run_play) * 1e3 / k)
                s.append(events_ms(torch, run_step) * 1e3 / k)
            say(f"{n:9d}   {spread(p)}   {spread(s)}   {statistics.median(p) / statistics.median(s):16.2f}")
        finally:
            a.close(), b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_play_step_probe.txt"))
    ap.add_argument("--train-steps", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--skip", choices=("on", "off", "both"), default="both")
    ap.add_argument("--only", default="1,2,3")
    args = ap.parse_args()
    rows = []

    def say(line=""):
        print(line, flush=True)
        rows.append(line)

    import torch

    import __graft_entry__ as ge
    ge.build()
    import gym2048_amd as g

    say(f"device: {torch.cuda.get_device_name(0)}")
    net = g.NTupleNet("4x6")
    trainer = g.Batched2048(1024, seed=11)
    try:
        trainer.reset()
        g.train(trainer, net, args.train_steps, 10)
    finally:
        trainer.close()
    say(f"network: \"4x6\" after train() of {args.train_steps} TD(0) steps on 1024 boards\n")
    only = set(args.only.split(","))
    if "1" in only:
        report_games(say, g, torch, net, ("on", "off") if args.skip == "both" else (args.skip,))
    if "2" in only:
        report_search(say, g, torch, net, args.parent_lib, max(5, args.reps))
    if "3" in only:
        report_step(say, g, torch, args.reps)
    with open(args.out, "w") as f:
        f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
