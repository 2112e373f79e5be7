"""CPU: the Monte-Carlo rollout search of g2048_device.h -- the header the kernel is compiled from -- built for the host
(tests/host_check/host_check.cpp, g++) and compared bit for bit with the pure-Python reference tests/mc_ref.py.  Every test
shows from the reference's own trace (never from the code under test) that its inputs reach the edge it is about."""
import numpy as np
import pytest

import mc_ref as ref
from analysis_helpers import (ONE_LEGAL, SEED, TERMINAL, high_boards, hm, host_mc, legal_count,  # noqa: F401 (hm: fixture)
                              random_boards, trajectory_boards)
from analysis_helpers import host_mc_split as host_split
from move_lut import build_row_lut


def check(lib, boards, R, L, seed=SEED, index_offset=0):
    """host == reference; returns the host result and the reference's trace counters."""
    stats = {}
    got = host_mc(lib, boards, R, L, seed, index_offset)
    want = ref.search_batch(boards, R, L, seed, index_offset, stats)
    bad = np.nonzero((got[0] != want[0]) | (got[1] != want[1]).any(1) | (got[2] != want[2]).any(1))[0]
    assert len(bad) == 0, f"{len(bad)} boards differ, first {np.asarray(boards)[bad[0]].tolist()}: " \
                          f"{[x[bad[0]].tolist() for x in got]} vs {[x[bad[0]].tolist() for x in want]}"
    return got, stats


def test_shift_row_is_the_row_table(oracle_lib):
    """The reference's move rule equals the oracle's shift() on every row of exponents 0..17 (tests/move_lut.py)."""
    out, score = build_row_lut(oracle_lib)
    rows = np.array(np.meshgrid(*[np.arange(18)] * 4, indexing="ij")).reshape(4, -1).T
    for k in range(0, len(rows), 7):
        new, s = ref.shift_row(tuple(int(x) for x in rows[k]))
        assert list(new) == out[k].tolist() and s == score[k], rows[k]


def test_reference_spawn_and_stream():
    """The reference's pieces by hand: spawn positions at both ends of the word, the 0.9 threshold, and the key tag."""
    b = (1, 0, 0, 2) + (3,) * 11 + (0,)
    assert ref.spawn(b, 0)[1] == 1 and ref.spawn(b, (1 << 32) - 1)[15] == 2       # first empty cell, a 2; last, a 4
    assert ref.spawn(b, (1 << 32) // 3 + 1)[2] in (1, 2) and ref.spawn(b, (1 << 32) // 3 + 1)[1] == 0
    w4, w2 = int(0.95 * 2 ** 32) // 3, int(0.5 * 2 ** 32) // 3                    # u * 3 = 0.95 and 0.5: cell 1, a 4 and a 2
    assert ref.spawn(b, w4)[1] == 2 and ref.spawn(b, w2)[1] == 1
    assert ref.spawn(b, w4 + (1 << 32) // 3 + 1)[2] == 2                           # u * 3 = 1.95: the second empty cell
    from oracle.cpu_ref import philox4x32_10
    assert ref.block(5, 7, 2, 3, 11) == philox4x32_10((11, 3, 7, 2), (5, ref.KEY_TAG))
    assert ref.block(5 | (9 << 32), 7, 2, 3, 11) == philox4x32_10((11, 3, 7, 2), (5, 9 ^ 0x4D435332))


def test_random_boards(hm):
    boards = random_boards(24, 1)
    _, stats = check(hm, boards, 5, 12)
    assert stats["cap"] > 0 and stats["terminal"] > 0, stats            # some playouts hit L, some end before it
    assert all(c > 0 for c in stats["candidates"]), stats              # some move needed the 2nd, 3rd and 4th candidate


def test_trajectory_boards_to_the_end(hm):
    """L large enough that every playout ends terminal: the whole random game after each root move."""
    boards = trajectory_boards(every=997)[:10]
    (_, val, stp), stats = check(hm, boards, 3, 65535)
    assert stats.get("cap", 0) == 0 and stats["terminal"] > 0, stats
    assert stp.max() > 3 * 50, stp.max()                                # long playouts: far more moves than a capped test
    assert all(c > 0 for c in stats["candidates"]), stats


def test_zero_one_legal_and_terminal(hm):
    assert legal_count(ONE_LEGAL)[0] == 1 and legal_count(TERMINAL)[0] == 0
    (act, val, stp), _ = check(hm, ONE_LEGAL, 7, 20)
    assert act[0] == 2 and (val[0, [0, 1, 3]] == -1).all() and (stp[0, [0, 1, 3]] == -1).all() and val[0, 2] >= 0 and stp[0, 2] > 0
    (act, val, stp), stats = check(hm, TERMINAL, 7, 20)
    assert act[0] == 0 and (val[0] == -1).all() and (stp[0] == -1).all() and stats == {}
    # full boards with a single merge: the root move leaves one empty cell, so playouts die early
    full = random_boards(400, 3)
    full = full[((full == 0).sum(1) == 0)]
    full = full[legal_count(full) >= 1][:6]
    assert len(full) >= 3
    _, stats = check(hm, full, 4, 30)
    assert stats["terminal"] > 0


def test_cap_one_and_one_rollout(hm):
    boards = random_boards(30, 4)
    (_, val, stp), stats = check(hm, boards, 6, 1)                      # L = 1: one move after the root move
    assert stats["cap"] > 0 and set(np.unique(stp[stp >= 0])) <= set(range(0, 7)) and stp.max() == 6
    (_, val, stp), stats = check(hm, boards, 1, 40)                     # R = 1
    assert stats["cap"] + stats.get("terminal", 0) == (val >= 0).sum()  # one playout per legal root move


@pytest.mark.parametrize("R", [3, 17, 67])
def test_rollouts_off_every_lane_count(hm, R):
    """R is no multiple of 4 or 16 (the kernel's lanes per direction)."""
    assert R % 4 and R % 16
    boards = np.concatenate([random_boards(3, 50 + R), trajectory_boards(every=1499)[:2]])
    check(hm, boards, R, 10, index_offset=1000 + R)


def test_index_and_seed_enter_the_stream(hm):
    boards = np.repeat(trajectory_boards(every=2003)[:1], 6, axis=0)     # equal boards at different rows
    (_, val, _), _ = check(hm, boards, 4, 30, index_offset=(1 << 32) - 6)  # the top of the 32-bit index range
    assert len({tuple(v) for v in val}) > 1
    other = host_mc(hm, boards, 4, 30, seed=SEED + (1 << 32))             # the high seed word matters
    assert (other[1] != val).any()
    assert np.array_equal(host_mc(hm, boards[2:], 4, 30, index_offset=(1 << 32) - 4)[1], val[2:])


def test_near_top_exponents(hm):
    """Exponents 26..31: merge scores past 2^31 wrap as the header states (mod 2^31 per move) and a direction's sum
    passes 2^32, which a 32-bit accumulator would lose."""
    boards = high_boards(6, 40, (2, 6))
    (_, val, _), _ = check(hm, boards, 8, 30)
    assert val.max() >= 1 << 32, val.max()


@pytest.mark.parametrize("K", [1, 3, 4, 16, 64])
def test_lane_split(hm, K):
    """The kernel's split (lane sub of K sums playouts sub, sub + K, ...; lanes added in another order) gives the same
    totals, for R below, equal to and above K and not a multiple of it."""
    boards = np.concatenate([random_boards(12, 7), trajectory_boards(every=1201)[:4], high_boards(2, 8, (2, 6))])
    for R in sorted({1, 3, K, K + 1, 2 * K + 3}):
        _, val, stp = host_mc(hm, boards, R, 25, index_offset=77)
        sval, sstp = host_split(hm, boards, R, 25, K, index_offset=77)
        assert np.array_equal(sval, val) and np.array_equal(sstp, stp), (K, R)


def test_limits_refused(hm):
    b = np.zeros((1, 16), np.uint8)
    out = np.zeros(8, np.int64)
    for R, L in ((0, 5), (65537, 5), (5, 0), (5, 65536)):
        assert hm.mc_check_boards(b.ctypes.data, 1, 0, R, L, 0, out.ctypes.data, out.ctypes.data, out.ctypes.data) == -1


def test_plays_ten_times_better_than_random_on_the_cpu(hm):
    """The definition itself meets the strength bar of the GPU test: whole games on the host build, the Monte-Carlo
    player (R = 16, playouts to the end) against the uniform random policy under the engine's rule (an illegal move ends
    the episode), 24 games each."""
    n = 24
    mc, rnd, moves = np.zeros(n, np.int64), np.zeros(4 * n, np.int64), np.zeros(4 * n, np.int64)
    assert hm.mc_check_play(n, 2048, 16, 65535, mc.ctypes.data, moves.ctypes.data) == 0   # never an illegal pick
    hm.mc_check_play(4 * n, 2048, 0, 1, rnd.ctypes.data, moves.ctypes.data)
    print(f"host games: mc R=16 mean {mc.mean():.1f}, random mean {rnd.mean():.1f}")
    assert mc.mean() >= 10 * rnd.mean(), (mc.mean(), rnd.mean())
