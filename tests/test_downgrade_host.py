"""CPU: downgrade_cells and ntuple_play_downgraded_step of g2048_device.h, compiled for the host (tests/host_downgrade), against
the reference model tests/downgrade_ref.py -- the rule on random and engineered boards with the properties the header claims for
it (checked with the oracle's move), and the step inside the fused player's loop against the oracle's step under the
references' evaluate on translated boards, bit for bit.  These tests fail without the feature: the header has neither
function to compile."""
import ctypes as C

import numpy as np
import pytest

import downgrade_ref as dref
import ntuple_play_ref as pref
import ntuple_staged_ref as sref
import oracle
from downgrade_helpers import (ENGINEERED, FLOOR_EXP, MIN_EXP, THR_3, engineered_rows, host_play, host_rule, load_host_downgrade,
                               random_boards, small_case, trace_of)
from ntuple_play_helpers import assert_same, budgets

SEED = 77
N = 64
RULES = [(5, 4), (1, 4), (15, 4), (11, 6), (8, 12), (31, 31), (16, 15)]


@pytest.fixture(scope="module")
def lib():
    return load_host_downgrade()


def test_the_two_models_agree():
    """The rule as the header words it (one board, plain Python) against the array form the other tests use."""
    boards = np.concatenate([random_boards(1500, 11), engineered_rows()[1]])
    for min_exp, floor_exp in RULES:
        out, k = dref.downgrade(boards, min_exp, floor_exp)
        for i, b in enumerate(boards):
            want, kk = dref.downgrade_one(b, min_exp, floor_exp)
            assert (out[i].tolist(), int(k[i])) == (want, kk), (b.tolist(), min_exp, floor_exp)


def test_engineered_boards(lib):
    """Every board gives the k worked out by hand, in the model and in the header's function; the high bits of a byte (the score
    bits of a record) change nothing and never reach the result."""
    names, boards, min_exp, floor_exp, k = engineered_rows()
    assert len(names) == len(ENGINEERED) >= 12
    noise = np.random.default_rng(3).integers(0, 8, boards.shape).astype(np.uint8) << 5
    for i, name in enumerate(names):
        want, kk = dref.downgrade_one(boards[i], int(min_exp[i]), int(floor_exp[i]))
        assert kk == k[i], f"{name}: the model gives k={kk}"
        assert want == [e - 1 if k[i] and e > k[i] else e for e in boards[i].tolist()], name
        for raw in (boards[i], boards[i] | noise[i]):
            out, missing = host_rule(lib, raw[None], int(min_exp[i]), int(floor_exp[i]))
            assert missing[0] == k[i] and out[0].tolist() == want, f"{name}: k={missing[0]} out={out[0].tolist()}"
    assert max(ENGINEERED["15, 16 and 17"][0]) == 17 and dref.downgrade_one(ENGINEERED["65536 at min_exp 15"][0], 15, 4)[0][0] == 15


def test_random_boards(lib):
    """120 000 boards of exponents 0..17 with random high bits under the rule of the play tests, 20 000 under each other rule."""
    boards = random_boards(120000, 5)
    assert ((boards >> 5) != 0).any() and (boards & 0x1f).max() == 17
    for j, (min_exp, floor_exp) in enumerate(RULES):
        part = boards if j == 0 else boards[20000 * (j - 1):20000 * j]
        want, k = dref.downgrade(part, min_exp, floor_exp)
        got, missing = host_rule(lib, part, min_exp, floor_exp)
        assert np.array_equal(missing, k) and np.array_equal(got, want), (min_exp, floor_exp, np.nonzero(missing != k)[0][:4])
        if (min_exp, floor_exp) in ((5, 4), (1, 4), (11, 6)):
            assert (k != 0).sum() > len(part) // 4 and (k == 0).sum() > 100      # both branches, often
    assert (host_rule(lib, boards[:20000], 31, 31)[1] == 0).all()


def _oracle_moves(lib_o, board):
    """[(legal, occupied cells after the move)] for the four directions, by the oracle's move on tile values."""
    out = []
    for d in range(4):
        M, sc = (C.c_int64 * 16)(*[(1 << int(e)) if e else 0 for e in board]), C.c_int64()
        legal = lib_o.g2048o_move(M, d, 0, C.byref(sc))
        out.append((bool(legal), tuple(v != 0 for v in M)))
    return out


def test_properties(lib):
    """A move is legal on the translated board exactly where it is legal on the board and leaves the same cells occupied; the
    translation is strictly increasing on the board's tiles; k is not on the board and k - 1 at most once."""
    lib_o = oracle.load()
    rng = np.random.default_rng(8)
    # boards as games make them: few distinct tiles, many empty cells, and dense ones
    sparse = np.where(rng.random((1500, 16)) < 0.45, 0, rng.integers(1, 13, (1500, 16))).astype(np.uint8)
    boards = np.concatenate([random_boards(1500, 9, high_bits=False), sparse, engineered_rows()[1]])
    moved = 0
    for min_exp, floor_exp in ((5, 4), (1, 4), (9, 6)):
        out, k = host_rule(lib, boards, min_exp, floor_exp)
        for b, t, kk in zip(boards.tolist(), out.tolist(), k.tolist()):
            if kk == 0:
                assert t == b
                continue
            moved += 1
            assert kk not in b and b.count(kk - 1) <= 1 and floor_exp <= kk < max(b) >= min_exp
            tiles = sorted(set(e for e in b if e))
            image = [t[b.index(e)] for e in tiles]
            assert all(x < y for x, y in zip(image, image[1:])) and all(t[c] == image[tiles.index(e)] for c, e in enumerate(b) if e)
            assert all((x == 0) == (y == 0) for x, y in zip(b, t))
            assert _oracle_moves(lib_o, b) == _oracle_moves(lib_o, t), (b, t)
    assert moved > 3000


# ------------------------------------------------------------------------------------------------ the step, in the player's loop
CASES = [("uniform", 2, 100), ("staged", 3, 100), ("mixed", 4, 100), ("mixed", 1, 60)]


@pytest.mark.parametrize("family, T, k", CASES, ids=[f"{f}-{T}" for f, T, _ in CASES])
def test_downgraded_play_is_the_model(lib, family, T, k):
    case = small_case(family, T)
    tr = trace_of(case, N, k, SEED)
    want = pref.limited(tr)
    on = tr.missing != 0
    assert on.sum() >= 100 and (tr.action[on] != tr.plain_action[on]).sum() >= 10, "the rule is at work and changes moves"
    assert want.moves == N * k
    if family != "uniform":
        low = dref.downgrade(tr.boards.reshape(-1, 16), MIN_EXP, FLOOR_EXP)[0]
        assert (sref.stage_batch(low[::7], THR_3) < sref.stage_batch(tr.boards.reshape(-1, 16)[::7], THR_3)).any(), "a translated board in an earlier stage"
    assert_same(host_play(lib, case, tr.start, SEED, tr.t0 + 1, k), want, case.name)


def test_budgets_and_the_identity_rule(lib):
    case, k = small_case("uniform", 2), 100
    tr = trace_of(case, N, k, SEED)
    left = budgets(N, 5)
    want = pref.limited(tr, left)
    assert pref.reaches(tr, want).ran_out
    assert_same(host_play(lib, case, tr.start, SEED, tr.t0 + 1, k, games_left=left), want, "budgets")
    # min_exp = 31 on boards that never hold 2^31: the plain player
    plain = pref.unlimited(pref.start_of(N, SEED), 40, case.rnet)
    assert_same(host_play(lib, case, plain.start, SEED, plain.t0 + 1, 40, min_exp=31), pref.limited(plain), "min_exp=31")


def test_a_bad_rule_is_refused(lib):
    for min_exp, floor_exp in ((0, 4), (32, 4), (5, 3), (5, 32)):
        assert lib.downgrade_check_rule(None, 0, min_exp, floor_exp, None, None) == -1
