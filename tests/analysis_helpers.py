"""Shared by the tests and probes of the analysis calls (afterstates, expectimax, Monte-Carlo search): the host build of
the search code (tests/host_check/host_check.cpp) behind ctypes, the board generators, periodic batches,
whole games under a policy, and the kernel constants the tests lean on.  A plain module: a test module that wants one of
the fixtures below imports it by name."""
import ctypes as C
import time

import numpy as np
import pytest

import mc_ref
import search_ref
from conftest import TRAJECTORIES, load_golden
from move_lut import build_row_lut

SEED = 0x0123456789ABCDEF   # of the Monte-Carlo tests
SEARCH_MAX_LANES = 1 << 24  # kSearchMaxLanes (g2048_kernels.hip): the grid cap past which the search kernels stride
WAVE_ROLLOUTS = 32          # kMcWaveRollouts: R >= this runs 64 lanes per board (16 per direction), below it 16 (4)
I32x4 = C.c_int32 * 4
ONE_LEGAL = np.array([[1, 2, 3, 4, 2, 3, 4, 5, 3, 4, 5, 6, 0, 0, 0, 0]], np.uint8)    # only "down" moves a tile
TERMINAL = np.array([[1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1]], np.uint8)


# ------------------------------------------------------------------------------------------------ the host build
def bind_analysis(lib):
    """Signatures of search_check_* and mc_check_* on libhost_check.so (as the ``host_check`` fixture loads it)."""
    P, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    for name, restype, argtypes in (("search_check_leaves", u64, [P, u64, u32]),
                                    ("search_check_heuristic", u32, [P, I32x4]),
                                    ("search_check_boards", C.c_int, [P, u64, u32, I32x4, P, P]),
                                    ("search_check_split", C.c_int, [P, u64, u32, I32x4, u32, P]),
                                    ("mc_check_boards", C.c_int, [P, u64, u32, u32, u32, u64, P, P, P]),
                                    ("mc_check_split", C.c_int, [P, u64, u32, u32, u32, u64, u32, P, P]),
                                    ("mc_check_play", u64, [u64, u64, u32, u32, P, P])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


def load_host_lib():
    """The bound library outside pytest (tools/, tests/fuzz_parity.py)."""
    import __graft_entry__ as ge
    return bind_analysis(C.CDLL(ge.build_host_check()))


@pytest.fixture(scope="module")
def hs(host_check):
    return bind_analysis(host_check)


hm = hs  # the same library: the expectimax tests call it hs, the Monte-Carlo tests hm


@pytest.fixture(scope="module")
def g(torch_cuda):
    import gym2048_amd
    return gym2048_amd


@pytest.fixture(scope="module")
def row_lut(oracle_lib):
    """shift() of every row of exponents 0..17 from the oracle's g2048o_shift, pinned against the reference's fixture
    (tests/move_lut.py)."""
    return build_row_lut(oracle_lib)


def _rows(boards):
    return np.ascontiguousarray(np.asarray(boards, np.uint8).reshape(-1, 16))


def host_search(lib, boards, depth, w=search_ref.DEFAULT_WEIGHTS):
    b = _rows(boards)
    act = np.zeros(len(b), np.uint8)
    val = np.zeros((len(b), 4), np.int32)
    assert lib.search_check_boards(b.ctypes.data, len(b), depth, I32x4(*w), act.ctypes.data, val.ctypes.data) == 0
    return act, val


def host_split(lib, boards, depth, K, w=search_ref.DEFAULT_WEIGHTS):
    b = _rows(boards)
    val = np.zeros((len(b), 4), np.int32)
    assert lib.search_check_split(b.ctypes.data, len(b), depth, I32x4(*w), K, val.ctypes.data) == 0
    return val


def host_mc(lib, boards, R, L, seed=SEED, index_offset=0):
    b = _rows(boards)
    act = np.zeros(len(b), np.uint8)
    val = np.zeros((len(b), 4), np.int64)
    stp = np.zeros((len(b), 4), np.int64)
    assert lib.mc_check_boards(b.ctypes.data, len(b), index_offset, R, L, seed, act.ctypes.data, val.ctypes.data, stp.ctypes.data) == 0
    return act, val, stp


def host_mc_split(lib, boards, R, L, K, seed=SEED, index_offset=0):
    b = _rows(boards)
    val = np.zeros((len(b), 4), np.int64)
    stp = np.zeros((len(b), 4), np.int64)
    assert lib.mc_check_split(b.ctypes.data, len(b), index_offset, R, L, seed, K, val.ctypes.data, stp.ctypes.data) == 0
    return val, stp


# ------------------------------------------------------------------------------------------------ boards
def random_boards(n, seed, max_exp=17):
    """Exponents 0..max_exp at densities from nearly empty to full."""
    rng = np.random.default_rng(seed)
    density = rng.uniform(0.05, 1.0, size=(n, 1))
    b = rng.integers(1, max_exp + 1, size=(n, 16))
    return np.where(rng.random((n, 16)) < density, b, 0).astype(np.uint8)


def high_boards(n, seed, empties, lo=26, hi=31, full_rows=0):
    """Exponents lo..hi with ``empties`` = (fewest, most) empty cells, a horizontal pair of ``hi`` (a merge makes hi + 1)
    and a vertical pair of a random exponent in every board; the first ``full_rows`` rows are all ``hi`` (merged twice:
    hi + 2; two such rows, merged a third time: hi + 3)."""
    rng = np.random.default_rng(seed)
    b = rng.integers(lo, hi + 1, size=(n, 16)).astype(np.uint8)
    for x in b:
        r, c = rng.integers(full_rows, 4), rng.integers(0, 3)
        keep = list(range(4 * full_rows)) + [4 * r + c, 4 * r + c + 1]
        x[keep] = hi
        r2, c2 = rng.integers(0, 3), rng.integers(0, 4)
        while 4 * r2 + c2 in keep or 4 * r2 + c2 + 4 in keep:
            r2, c2 = rng.integers(0, 3), rng.integers(0, 4)
        x[[4 * r2 + c2, 4 * r2 + c2 + 4]] = rng.integers(lo, hi + 1)
        keep = set(keep) | {4 * r2 + c2, 4 * r2 + c2 + 4}
        free = [k for k in range(16) if k not in keep]
        x[rng.choice(free, int(rng.integers(empties[0], empties[1] + 1)), replace=False)] = 0
    return b


def trajectory_boards(every=1):
    out = [load_golden(t)["boards"].reshape(-1, 16)[::every] for t in TRAJECTORIES]
    return np.unique(np.concatenate(out), axis=0)


def mid_game(m, seed, max_empty=16):
    """m distinct boards of the golden trajectories with at most ``max_empty`` empty cells."""
    traj = trajectory_boards()
    traj = traj[(traj == 0).sum(1) <= max_empty]
    return traj[np.random.default_rng(seed).choice(len(traj), m, replace=False)]


def mixed_boards(n, seed):
    boards = random_boards(n, seed)
    traj = trajectory_boards(every=3)
    boards[::2] = traj[np.random.default_rng(seed).integers(0, len(traj), len(boards[::2]))]
    return boards


def afterstate_empties(boards):
    """int [n, 4]: empty cells of move(b, d) by the expectimax reference, 0 where d is illegal."""
    out = np.zeros((len(boards), 4), np.int64)
    for i, b in enumerate(np.asarray(boards).reshape(-1, 16)):
        for d in range(4):
            a, legal = search_ref.move(tuple(int(x) % 32 for x in b), d)
            out[i, d] = sum(1 for x in a if x == 0) if legal else 0
    return out


def legal_count(boards):
    """Legal moves of every board by the Monte-Carlo reference."""
    return np.array([sum(mc_ref.move(tuple(int(x) % 32 for x in b), d)[2] for d in range(4))
                     for b in np.asarray(boards).reshape(-1, 16)])


# ------------------------------------------------------------------------------------------------ periodic batches
def tiled(torch, base, n):
    """uint8 [n, 16] on the device: row i = base[i % m]."""
    b = torch.as_tensor(np.ascontiguousarray(base, dtype=np.uint8)).cuda()
    return b.repeat(-(-n // len(b)), 1)[:n]


def assert_rows_periodic(torch, got, want, chunk):
    """got[i] == want[i % m] for every row i, compared on the device ``chunk`` rows at a time."""
    m, n = len(want), len(got)
    for k in range(0, n, chunk):
        part = got[k:k + chunk]
        idx = torch.arange(k, k + len(part), device=got.device) % m
        eq = (part == want[idx]).reshape(len(part), -1).all(1)
        if not bool(eq.all()):
            i = k + int((~eq).nonzero()[0, 0])
            raise AssertionError(f"row {i} (base row {i % m}) differs: {got[i].flatten()[:16].tolist()} vs "
                                 f"{want[i % m].flatten()[:16].tolist()}")


# ------------------------------------------------------------------------------------------------ whole games
def random_policy(torch, n, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return lambda eng, t: torch.randint(0, 4, (n,), generator=gen, device="cuda", dtype=torch.uint8)


def play(g, torch, n, seed, choose, cap=5000):
    """Every board's first game on a numpy-RNG engine, move t chosen by ``choose(eng, t)``: (final scores, -1 for a game
    unfinished at the cap; whether a chosen move of a running game was illegal; moves played by all boards; seconds)."""
    eng = g.Batched2048(n, seed=seed, rng="numpy")
    first = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    illegal, moves = False, 0
    try:
        eng.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(cap):
            eng.step(choose(eng, t))
            live = first < 0
            moves += int(live.sum())
            illegal |= bool((eng.illegal.bool() & live).any())
            ended = eng.terminated.bool() & live
            if bool(ended.any()):
                first[ended] = eng.last_scores().to(torch.int64)[ended]
            if not bool((first < 0).any()):
                break
        torch.cuda.synchronize()
        return first.cpu().numpy(), illegal, moves, time.perf_counter() - t0
    finally:
        eng.close()
