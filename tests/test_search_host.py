"""CPU: the expectimax code of g2048_device.h -- the header the search kernels are compiled from -- built for the host
(tests/host_search/search_check.cpp, g++) and compared bit for bit with the pure-Python reference tests/search_ref.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import search_ref as ref
from conftest import ROOT, TRAJECTORIES, load_golden

SRC = os.path.join(ROOT, "tests", "host_search", "search_check.cpp")
I32x4 = C.c_int32 * 4


def build_search_check(out_dir):
    so = os.path.join(str(out_dir), "libsearch_check.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, SRC])
    lib = C.CDLL(so)
    lib.search_check_heuristic.restype = C.c_uint32
    lib.search_check_heuristic.argtypes = [C.c_void_p, I32x4]
    lib.search_check_boards.restype = C.c_int
    lib.search_check_boards.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, I32x4, C.c_void_p, C.c_void_p]
    lib.search_check_split.restype = C.c_int
    lib.search_check_split.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, I32x4, C.c_uint32, C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def hs(tmp_path_factory):
    return build_search_check(tmp_path_factory.mktemp("search_check"))


def host_search(lib, boards, depth, w=ref.DEFAULT_WEIGHTS):
    b = np.ascontiguousarray(np.asarray(boards, np.uint8).reshape(-1, 16))
    act = np.zeros(len(b), np.uint8)
    val = np.zeros((len(b), 4), np.int32)
    assert lib.search_check_boards(b.ctypes.data, len(b), depth, I32x4(*w), act.ctypes.data, val.ctypes.data) == 0
    return act, val


def host_split(lib, boards, depth, K, w=ref.DEFAULT_WEIGHTS):
    b = np.ascontiguousarray(np.asarray(boards, np.uint8).reshape(-1, 16))
    val = np.zeros((len(b), 4), np.int32)
    assert lib.search_check_split(b.ctypes.data, len(b), depth, I32x4(*w), K, val.ctypes.data) == 0
    return val


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


def afterstate_empties(boards):
    """int [n, 4]: empty cells of move(b, d) by the Python reference, 0 where d is illegal."""
    out = np.zeros((len(boards), 4), np.int64)
    for i, b in enumerate(np.asarray(boards).reshape(-1, 16)):
        for d in range(4):
            a, legal = ref.move(tuple(int(x) % 32 for x in b), d)
            out[i, d] = sum(1 for x in a if x == 0) if legal else 0
    return out


def trajectory_boards(every=1):
    out = [load_golden(t)["boards"].reshape(-1, 16)[::every] for t in TRAJECTORIES]
    return np.unique(np.concatenate(out), axis=0)


def check(lib, boards, depth, w=ref.DEFAULT_WEIGHTS):
    act, val = host_search(lib, boards, depth, w)
    ract, rval = ref.search_batch(boards, depth, w)
    bad = np.nonzero((act != ract) | (val != rval).any(1))[0]
    assert len(bad) == 0, f"{len(bad)} boards differ, first {boards[bad[0]].tolist()}: {act[bad[0]]} {val[bad[0]]} " \
                          f"vs {ract[bad[0]]} {rval[bad[0]]}"
    return act, val


def test_heuristic(hs):
    boards = random_boards(2000, 1, max_exp=31)
    for w in (ref.DEFAULT_WEIGHTS, (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1 << 24, 65535, 65535, 65535)):
        for b in boards:
            assert hs.search_check_heuristic(np.ascontiguousarray(b).ctypes.data, I32x4(*w)) == ref.heuristic(tuple(int(x) for x in b), w)


def test_heuristic_bound():
    """H < 2^27 at the largest weights, on the worst line the exponents allow (34 = 31 + three merges)."""
    worst = (34, 33, 34, 33) * 4
    assert ref.heuristic(worst, (1 << 24, 65535, 65535, 65535)) < 1 << 27
    assert ref.heuristic((0,) * 16, (1 << 24, 65535, 65535, 65535)) < 1 << 27


def test_depth1_random(hs):
    check(hs, random_boards(3000, 2), 1)


def test_depth1_trajectories(hs):
    boards = trajectory_boards(every=7)
    assert len(boards) > 1000
    check(hs, boards, 1)


def test_depth1_weights_and_mod32(hs):
    boards = random_boards(400, 3, max_exp=31)
    check(hs, boards, 1, (1 << 24, 65535, 65535, 65535))
    check(hs, boards, 1, (0, 0, 0, 0))
    check(hs, boards, 1, (7, 3, 65535, 1))
    # the plain form takes exponents mod 32 (g2048_afterstates_plain)
    hi = boards | np.where(boards > 0, 32, 0).astype(np.uint8)
    assert all(np.array_equal(x, y) for x, y in zip(host_search(hs, hi, 1), host_search(hs, boards, 1)))


def test_depth2(hs):
    boards = np.concatenate([random_boards(24, 4), trajectory_boards(every=997)[:16]])
    assert len(boards) >= 32
    check(hs, boards, 2)
    check(hs, boards[:8], 2, (1 << 24, 65535, 65535, 65535))


def test_depth3(hs):
    rng = np.random.default_rng(5)
    boards = random_boards(200, 6)
    boards = boards[(boards == 0).sum(1) <= 6][:4]  # few empty cells keep the Python tree small
    boards = np.concatenate([boards, trajectory_boards(every=1)[rng.integers(0, 1000, 1)]])
    check(hs, boards, 3)


@pytest.mark.parametrize("name", sorted(ref.HAND_CASES))
def test_hand_cases(hs, name):
    board, depth, w, expected = ref.HAND_CASES[name]
    act, val = check(hs, board[None], depth, w)
    if expected is not None:
        assert act[0] == expected
    if name == "dead":
        assert (val[0] == -1).all()
    if name == "one_legal_move":
        assert (val[0] >= 0).sum() == 1
    if name == "tie_right_left":
        assert val[0, 1] == val[0, 3] >= 0 and val[0, 0] == val[0, 2] == -1
    if name == "empty_from_merge":
        assert (board == 0).sum() == 0 and (val[0] >= 0).any()
    if name == "zero_weights":
        assert (val[0][val[0] >= 0] == 0).all()
    for d in range(1, 4) if name != "max_weights" else (1,):
        check(hs, board[None], d, w)


@pytest.mark.parametrize("depth,K", [(1, 4), (1, 16), (2, 16), (2, 3), (3, 16)])
def test_lane_split(hs, depth, K):
    """The kernels' split (K lanes per direction, partial sums added before the one divide) gives the same values."""
    boards = random_boards({1: 500, 2: 40, 3: 3}[depth], 7)
    if depth == 3:
        boards = boards[(boards == 0).sum(1) <= 6][:2]
    _, val = host_search(hs, boards, depth)
    assert np.array_equal(host_split(hs, boards, depth, K), val)


@pytest.mark.parametrize("w", [ref.DEFAULT_WEIGHTS, ref.MAX_WEIGHTS], ids=["default", "max"])
def test_near_top_exponents_depth2_depth3(hs, w):
    """Exponents 26..31 with equal neighbours: the merges inside the tree make exponents 32..34, which the byte tricks of
    line_terms / shift4 must carry (the header's claim).  Depth 2 on 12 boards, depth 3 on 3 (few empty cells)."""
    b2 = np.concatenate([high_boards(6, 40, (1, 5)), high_boards(6, 42, (1, 4), full_rows=1)])
    b3 = high_boards(2, 41, (1, 3), full_rows=2)
    check(hs, b2, 2, w)
    check(hs, b3, 3, w)
    # the inputs reach the edge: every tree goes past 31, the depth-2 trees to 33, the depth-3 trees to 34
    tops2, tops3 = [ref.max_exponent(b, 2) for b in b2], [ref.max_exponent(b, 3) for b in b3]
    assert min(tops2) >= 32 and max(tops2) == 33 and tops3 == [34] * len(b3), (tops2, tops3)


@pytest.mark.parametrize("depth,n", [(2, 40), (3, 3)])
def test_lane_split_wide_sums(hs, depth, n):
    """The kernels' split at K = 16 with the largest weights, where a root's chance sum is wider than 32 bits: the
    64-bit partial sums of 16 lanes must add up to the one-lane sum."""
    boards = high_boards(n, 50 + depth, (6, 10))
    _, val = host_search(hs, boards, depth, ref.MAX_WEIGHTS)
    assert np.array_equal(host_split(hs, boards, depth, 16, ref.MAX_WEIGHTS), val)
    E = afterstate_empties(boards)
    # value = floor(total / 10E), so value * 10E <= total: these roots summed past 2^32
    wide = (val >= 0) & (val.astype(np.int64) * 10 * E >= 1 << 32)
    assert wide.sum() * 4 >= (val >= 0).sum(), (wide.sum(), (val >= 0).sum())
    if depth == 2:  # the undivided sums themselves, from the Python reference
        totals = [ref.root_totals(b, 2, ref.MAX_WEIGHTS) for b in boards[:6]]
        assert max(t for row in totals for t in row if t is not None) >= 1 << 32
        for row, v, e in zip(totals, val, E):
            assert [-1 if t is None else t // (10 * k) for t, k in zip(row, e)] == v.tolist()
