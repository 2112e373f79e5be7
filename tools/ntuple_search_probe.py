"""Cost and playing strength of the n-tuple expectimax (g2048_ntuple_search) on MI355X; writes
profiles/r12_ntuple_search_probe.txt.

Time: microseconds per launch of g2048_ntuple_search_plain (HIP events around each launch, two warm-up launches, at least
five timed ones, both outputs) at depths 1 and 2 for 2^12 and 2^16 boards (and 2^20 at depth 1), the 4x6 and 17x4 nets
with random weights, on mid-game boards (games of the depth-1 expectimax player of §7, 150 moves in) and random-rollout
boards (200 random moves in), with the network evaluations (leaves, counted by a torch expansion of the tree's shape on a
sample) per second.
Baseline: the depth-1 result composed from calls that exist without the kernel -- g2048_afterstates_plain, the child
boards of every empty cell built in torch (compacted to the real children), g2048_ntuple_evaluate_plain on them, and a
torch reduction with a floor division -- checked equal to the kernel's output first.
Strength: the 4x6 net after the 50 000 TD steps of §9 (same seeds), 512 games each for the greedy player, depth 1 and
depth 2: mean score and the share of games whose largest tile reached 2048.

  python tools/ntuple_search_probe.py [--out FILE] [--no-strength] [--lib PATH]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SHAPES = ("4x6", "17x4")
SIZES = {1: (1 << 12, 1 << 16, 1 << 20), 2: (1 << 12, 1 << 16)}
GAMES = 512
ILLEGAL = -(1 << 63)


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


def children(g, torch, boards):
    """The real chance children of every legal afterstate of plain boards [n, 16]: (afterstates result, child boards
    [M, 16], their weight 9 / 1 [M], their (board, direction) slot [M] in 0..4n-1, empty cells per slot [4n])."""
    a = g.afterstates(boards)
    n = len(boards)
    after = a.boards.reshape(4 * n, 16)
    legal = ((a.legal.unsqueeze(1) >> torch.arange(4, device=boards.device)) & 1).bool().reshape(4 * n)
    empty = (after == 0) & legal.unsqueeze(1)                          # [4n, 16]
    slot, cell = empty.nonzero(as_tuple=True)
    kids = after[slot].repeat_interleave(2, 0)                         # [2M', 16]: spawn 2, spawn 4
    exponent = torch.tensor([1, 2], dtype=torch.uint8, device=boards.device).repeat(len(slot))
    kids[torch.arange(len(kids), device=boards.device), cell.repeat_interleave(2)] = exponent
    weight = torch.tensor([9, 1], dtype=torch.int64, device=boards.device).repeat(len(slot))
    return a, kids, weight, slot.repeat_interleave(2), empty.sum(1)


def composed_depth1(g, torch, net, boards):
    """value [n, 4] and action [n] of depth 1 from afterstates, a torch child expansion, evaluate and a torch reduction."""
    a, kids, weight, slot, empties = children(g, torch, boards)
    n = len(boards)
    best = net.evaluate(kids.contiguous(), out=g.NTupleEval(None, None, torch.empty(len(kids), dtype=torch.int64, device=boards.device),
                                                             None, None)).best
    total = torch.zeros(4 * n, dtype=torch.int64, device=boards.device).index_add_(0, slot, weight * best)
    chance = torch.div(total, (10 * empties).clamp(min=1), rounding_mode="floor")
    legal = ((a.legal.unsqueeze(1) >> torch.arange(4, device=boards.device)) & 1).bool()
    value = torch.where(legal, (a.score.to(torch.int64) << net.frac_bits) + chance.reshape(n, 4), ILLEGAL)
    # the smallest d of largest value: argmax returns the first maximum; an all-illegal row gives 0
    return value, value.argmax(1).to(torch.uint8)


def leaves_per_board(g, torch, boards, depth):
    """Mean network evaluations (legal leaf moves) per board of the depth-`depth` tree, counted on a sample in torch."""
    frontier = boards
    for _ in range(depth):
        frontier = children(g, torch, frontier)[1]
    legal = g.afterstates(frontier.contiguous()).legal
    count = sum(((legal >> d) & 1).sum().item() for d in range(4))
    return count / len(boards)


def boards_of(g, torch, n, kind):
    """n boards of games in progress: "mid" = the depth-1 expectimax player 150 moves in, "random" = 200 random moves in."""
    eng = g.Batched2048(n, seed=7)
    try:
        eng.reset()
        if kind == "random":
            eng.rollout_random(200)
        else:
            act = torch.empty(n, dtype=torch.uint8, device="cuda")
            for _ in range(150):
                eng.expectimax(1, out=g.Search(act, None))
                eng.step(act)
        return eng.boards().reshape(-1, 16).clone()
    finally:
        eng.close()


def games(g, torch, choose, n=GAMES, seed=2048, cap=50000):
    """Every board's first game on a numpy-RNG engine: (scores, largest exponent of the terminal board, moves of all games)."""
    eng = g.Batched2048(n, seed=seed, rng="numpy")
    score = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    top = torch.zeros(n, dtype=torch.int64, device="cuda")
    moves = 0
    try:
        eng.reset()
        for _ in range(cap):
            eng.step(choose(eng), auto_reset=True, want_info=True)
            live = score < 0
            moves += int(live.sum())
            ended = eng.terminated.bool() & live
            if bool(ended.any()):
                score[ended] = eng.last_scores().to(torch.int64)[ended]
                top[ended] = eng.terminal_boards[ended].max(1).values.to(torch.int64)
            if not bool((score < 0).any()):
                break
        return score.cpu().numpy(), top.cpu().numpy(), moves
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_ntuple_search_probe.txt"))
    ap.add_argument("--no-strength", action="store_true")
    ap.add_argument("--lib", default=None, help="another build of the library (a lane-group variant) to time instead")
    args = ap.parse_args()
    rows = []

    def say(line=""):
        print(line, flush=True)
        rows.append(line)

    import torch

    import gym2048_amd as g
    from gym2048_amd import _lib
    if args.lib:
        _lib.LIB_PATH = args.lib
    else:
        import __graft_entry__ as ge
        ge.build()
    say(f"device: {torch.cuda.get_device_name(0)}; library {os.path.basename(_lib.LIB_PATH)}")
    gen = torch.Generator(device="cuda").manual_seed(1)
    sets = {kind: boards_of(g, torch, 1 << 20, kind) for kind in ("mid", "random")}
    for kind, b in sets.items():
        say(f"{kind} boards: {(b == 0).sum(1).float().mean().item():.1f} empty cells on average")
    nets = {}
    for shape in SHAPES:
        nets[shape] = g.NTupleNet(shape)
        nets[shape].weights.copy_(torch.randint(-(1 << 20), 1 << 20, nets[shape].weights.shape, generator=gen, device="cuda",
                                                dtype=torch.int32))
    say("\nsearch: us per launch (action and value; HIP events, 2 warm-up launches, >= 5 timed), leaves = network evaluations")
    say("depth shape  boards        n  leaves/board  us/launch  Gleaves/s  Ggathers/s")
    for depth, sizes in SIZES.items():
        for shape, net in nets.items():
            for kind, b in sets.items():
                leaves = leaves_per_board(g, torch, b[:256 if depth == 2 else 4096].contiguous(), depth)
                for n in sizes:
                    x = b[:n].contiguous()
                    out = net.search(x, depth)
                    us = timed(torch, lambda: net.search(x, depth, out=out))
                    say(f"{depth:5d} {shape:5s} {kind:7s} {n:8d} {leaves:13.0f} {us:10.1f} {n * leaves / us / 1e3:10.2f} "
                        f"{n * leaves * 8 * net.n_tuples / us / 1e3:11.1f}")
    say("\nbaseline, depth 1: afterstates + torch child expansion (compacted) + ntuple_evaluate + torch reduction, equal to the kernel")
    say("shape  boards        n  kernel us  composed us  composed / kernel")
    for shape, net in nets.items():
        for kind, b in sets.items():
            for n in (1 << 12, 1 << 16):
                x = b[:n].contiguous()
                out = net.search(x, 1)
                value, action = composed_depth1(g, torch, net, x)
                assert torch.equal(value, out.value) and torch.equal(action, out.action), "composition != kernel"
                k_us = timed(torch, lambda: net.search(x, 1, out=out))
                c_us = timed(torch, lambda: composed_depth1(g, torch, net, x), min_reps=3)
                say(f"{shape:5s} {kind:7s} {n:8d} {k_us:10.1f} {c_us:12.1f} {c_us / k_us:18.1f}")
    if not args.no_strength:
        import numpy as np
        say(f"\nstrength: 4x6 net, train() 50 000 TD steps from zero weights (1 024 boards, seed 11, lr_shift 10: §9), then "
            f"{GAMES} games each (numpy-RNG engine, seed 2048)")
        say("player    mean score   median      max  reached 2048  mean moves  seconds")
        net = g.NTupleNet("4x6")
        eng = g.Batched2048(1024, seed=11)
        try:
            eng.reset()
            g.train(eng, net, 50000, 10)
        finally:
            eng.close()
        act = torch.empty(GAMES, dtype=torch.uint8, device="cuda")
        players = {"greedy": lambda e: e.ntuple_evaluate(net, out=g.NTupleEval(None, act, None, None, None)).action,
                   "depth 1": lambda e: e.ntuple_search(net, 1, out=g.NTupleSearch(act, None)).action,
                   "depth 2": lambda e: e.ntuple_search(net, 2, out=g.NTupleSearch(act, None)).action}
        for name, choose in players.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            score, top, moves = games(g, torch, choose)
            dt = time.perf_counter() - t0
            ok = score >= 0
            say(f"{name:8s} {score[ok].mean():11.1f} {np.median(score[ok]):8.0f} {score[ok].max():8d} {100.0 * (top[ok] >= 11).mean():11.1f}% "
                f"{moves / GAMES:11.1f} {dt:8.1f}" + ("" if ok.all() else f" ({(~ok).sum()} games unfinished at the cap)"))
    with open(args.out, "w") as f:
        f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
