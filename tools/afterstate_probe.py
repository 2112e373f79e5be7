#!/usr/bin/env python
"""afterstate_probe.py -- measurement tool for g2048_afterstates (not part of the suite).

    python tools/afterstate_probe.py [--mode time|trace|pmc] [--points 2p20,2p24,u8,f16,f32] [--json OUT]

Boards: a seeded engine after 64 random steps (live mid-game boards).  Per point, three ways to get every board's four
afterstates (+ scores, legality mask, optionally the one-hot of each):
  engine   g2048_afterstates on the engine's records (one launch)
  plain    g2048_afterstates_plain on the same boards as plain uint8[n][16] (one launch)
  compose  what a caller had to do without it: per direction set_boards into a scratch engine + g2048_move +
           get_boards (+ g2048_onehot), then interleaving copies into the [n][4] layout and the mask from the four flags
--mode time: HIP events around back-to-back calls (window >= --window s, calibrated), the three alternated in the same
  process for --rounds rounds; median us per call, and the algorithmic bytes per board over that time vs 8 TB/s:
  16 B read + 64 (afterstates) + 16 (scores) + 1 (mask) = 97 B per board, + 1 024 / 2 048 / 4 096 B of observation.
--mode trace: a few calls of each, for `rocprofv3 --kernel-trace --stats -- python tools/afterstate_probe.py --mode trace`.
--mode pmc: engine form only, for a `rocprofv3 --pmc FETCH_SIZE WRITE_SIZE` run of its own.
--summary KERNEL_TRACE_CSV [--pmc-csv COUNTER_CSV]: no GPU; per afterstates_kernel instantiation and grid size, the mean
  dispatch time of the trace, the fraction of the 8 TB/s peak on the byte model, and (with the counter CSV) the measured
  FETCH_SIZE / WRITE_SIZE per board against the model.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

POINTS = {  # name: (log2 boards, obs dtype)
    "2p20": (20, None), "2p24": (24, None), "u8": (20, torch.uint8), "f16": (20, torch.float16), "f32": (20, torch.float32),
}
OBS_BYTES = {None: 0, torch.uint8: 1024, torch.float16: 2048, torch.float32: 4096}
PEAK = 8e12


class Point:
    def __init__(self, log2n, obs_dtype):
        from gym2048_amd import _lib
        from gym2048_amd.batched import Batched2048, _OBS_DTYPES, _afterstate_io
        self.lib = _lib.load()
        n = self.n = 1 << log2n
        self.obs_dtype = obs_dtype
        dev = torch.device("cuda", 0)
        self.eng = Batched2048(n, seed=42)
        self.eng.reset(seed=42)
        self.eng.rollout_random(64)
        self.boards = self.eng.boards().view(n, 16)
        self.io, self.out = _afterstate_io(n, dev, obs_dtype, None)
        # composition buffers
        self.scratch = Batched2048(n)
        self.acts = [torch.full((n,), d, dtype=torch.uint8, device=dev) for d in range(4)]
        self.c_boards = torch.empty((4, n, 16), dtype=torch.uint8, device=dev)
        self.c_score = torch.empty((4, n), dtype=torch.int32, device=dev)
        self.c_legal = torch.empty((4, n), dtype=torch.uint8, device=dev)
        self.c_obs = None if obs_dtype is None else torch.empty((4, n, 16, 4, 4), dtype=obs_dtype, device=dev)
        self.c_obs_code = None if obs_dtype is None else _OBS_DTYPES[obs_dtype]
        self.shifts = torch.tensor([1, 2, 4, 8], dtype=torch.uint8, device=dev).view(4, 1)
        _, self.c_out = _afterstate_io(n, dev, obs_dtype, None)
        self.stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        self.bytes = n * (97 + OBS_BYTES[obs_dtype])

    def engine(self):
        self.lib.g2048_afterstates(self.eng._h, C.byref(self.io), self.stream)

    def plain(self):
        self.lib.g2048_afterstates_plain(self.boards.data_ptr(), self.n, C.byref(self.io), self.stream)

    def compose(self):
        lib, h, s = self.lib, self.scratch._h, self.stream
        for d in range(4):
            lib.g2048_set_boards(h, self.boards.data_ptr(), s)
            lib.g2048_move(h, self.acts[d].data_ptr(), 1, 0, self.c_score[d].data_ptr(), self.c_legal[d].data_ptr(), s)
            lib.g2048_get_boards(h, self.c_boards[d].data_ptr(), s)
            if self.c_obs is not None:
                lib.g2048_onehot(h, self.c_obs[d].data_ptr(), self.c_obs_code, s)
        o = self.c_out
        o.boards.copy_(self.c_boards.transpose(0, 1))
        o.score.copy_(self.c_score.t())
        torch.sum(self.c_legal * self.shifts, dim=0, dtype=torch.uint8, out=o.legal)
        if self.c_obs is not None:
            o.obs.copy_(self.c_obs.transpose(0, 1))

    def check(self):
        self.engine()
        self.compose()
        torch.cuda.synchronize()
        for name in ("boards", "score", "legal", "obs"):
            a, b = getattr(self.out, name), getattr(self.c_out, name)
            assert (a is None) == (b is None) and (a is None or torch.equal(a, b)), name

    def close(self):
        self.eng.close()
        self.scratch.close()


def time_calls(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / reps  # us per call


def calibrate(fn, window):
    reps = 1
    while True:
        us = time_calls(fn, reps)
        if us * reps >= window * 1e6:
            return reps
        reps = max(reps * 2, int(reps * window * 1e6 / max(us * reps, 1.0) * 1.2))


def summarize(trace_csv, pmc_csv=None):
    """Per (afterstates_kernel instantiation, boards): mean kernel-trace time, fraction of peak on the byte model."""
    import csv
    import re
    obs_bytes = {"true": None, "false": 0}
    groups = {}
    for r in csv.DictReader(open(trace_csv)):
        name = r.get("Kernel_Name", "")
        if "afterstates_kernel" not in name:
            continue
        boards = int(r["Grid_Size_X"]) if "Grid_Size_X" in r else int(r["Grid_Size"])
        ns = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        flags = tuple(re.search(r"afterstates_kernel<([^>]*)>", name).group(1).split(", "))  # (PLAIN, [STAGED,] OBS)
        groups.setdefault((flags, boards), []).append(ns)
    print("kernel                                  boards      calls  mean_us  bytes/board  frac_8TB/s")
    for (flags, boards), v in sorted(groups.items()):
        us = sum(v) / len(v) / 1e3
        per = 97 if obs_bytes[flags[-1]] == 0 else None
        frac = f"{per * boards / (us * 1e-6) / PEAK:.3f}" if per else "(obs: see dtype)"
        print(f"afterstates_kernel<{', '.join(flags)}>  {boards:>10} {len(v):>6} {us:>8.2f}  {per or '97+obs':>11}  {frac}")
    if pmc_csv:
        print("\ncounters (engine form, afterstates_kernel only): bytes per board")
        for r in csv.DictReader(open(pmc_csv)):
            if "afterstates_kernel" in r.get("Kernel_Name", ""):
                boards = int(r["Grid_Size"]) if "Grid_Size" in r else int(r.get("Grid_Size_X", 0))
                print(f"  {r['Counter_Name']:<11} {float(r['Counter_Value']):>16.0f} B = {float(r['Counter_Value']) / boards:7.2f} B/board"
                      f"  (model: read 16, write 81)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("time", "trace", "pmc"), default="time")
    ap.add_argument("--points", default=",".join(POINTS))
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json")
    ap.add_argument("--summary")
    ap.add_argument("--pmc-csv")
    args = ap.parse_args()
    if args.summary:
        return summarize(args.summary, args.pmc_csv)
    import __graft_entry__ as ge
    ge.build_hip()
    rows = []
    for name in args.points.split(","):
        log2n, dt = POINTS[name]
        p = Point(log2n, dt)
        if args.mode == "pmc":
            for _ in range(3):
                p.engine()
            torch.cuda.synchronize()
            p.close()
            continue
        p.check()                                      # the one launch computes what the composition computes
        if args.mode == "trace":
            for _ in range(10):
                p.engine()
                p.plain()
            for _ in range(3):
                p.compose()
            torch.cuda.synchronize()
            p.close()
            continue
        fns = {"engine": p.engine, "plain": p.plain, "compose": p.compose}
        reps = {}
        for k, fn in fns.items():                      # warm-up + calibration of the window
            time_calls(fn, 3)
            reps[k] = calibrate(fn, args.window)
        samples = {k: [] for k in fns}
        for _ in range(args.rounds):                   # alternated in the same process
            for k, fn in fns.items():
                samples[k].append(time_calls(fn, reps[k]))
        med = {k: statistics.median(v) for k, v in samples.items()}
        row = dict(point=name, boards=p.n, obs=str(dt).replace("torch.", "") if dt else None,
                   bytes_per_board=97 + OBS_BYTES[dt], reps=reps,
                   us={k: round(v, 2) for k, v in med.items()},
                   us_min_max={k: [round(min(v), 2), round(max(v), 2)] for k, v in samples.items()},
                   frac_peak={k: round(p.bytes / (med[k] * 1e-6) / PEAK, 3) for k in ("engine", "plain")},
                   speedup_vs_compose={k: round(med["compose"] / med[k], 2) for k in ("engine", "plain")})
        rows.append(row)
        print(json.dumps(row), flush=True)
        p.close()
        torch.cuda.empty_cache()
    if args.json and rows:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
