"""CPU: ntuple_play_step of g2048_device.h inside the fused player's loop, compiled for the host (tests/host_ntuple_play),
against the reference model tests/ntuple_play_ref.py -- the oracle's step under the references' evaluate -- bit for bit: the
records with their score-deficit bits, the terminated flag and the action of every step, the episode counts, the return sum,
the histogram, the move count, the terminal records and the budgets.  Every test first shows from the reference's own
trace (never from the code under test) that its run reaches what it names.  These tests fail without the feature: the
header has no ntuple_play_step to compile."""
import numpy as np
import pytest

import late_game as lg
import ntuple_play_ref as pref
import ntuple_staged_ref as sref
from ntuple_play_helpers import (THR_3, assert_same, budgets, engineered_trace, host_run, load_host_play, mixed_case, staged_case, trace_of,
                                 uniform_case)

SEED = 77
N = 64
# steps per network: the fewest after which the reference's trace holds what the tests name (several boards have finished a
# second game; under the zero net, whose games are longer, a first one) -- the pure-Python reference costs ~0.6 ms per move
CASES = {"17x4": (uniform_case, 130), "staged": (staged_case, 160), "mixed": (mixed_case, 115), "zero": (lambda: uniform_case(zero=True), 130)}


@pytest.fixture(scope="module")
def lib():
    return load_host_play()


def run_of(name):
    make, k = CASES[name]
    case = make()
    return case, k, trace_of(case, N, k, SEED)


@pytest.mark.parametrize("name", sorted(CASES))
def test_unlimited_play_is_the_composition(lib, name):
    case, k, tr = run_of(name)
    want = pref.limited(tr)
    hit = pref.reaches(tr, want)
    assert hit.one_episode and hit.directions == {0, 1, 2, 3} and want.moves == N * k
    if name != "zero":
        assert hit.two_episodes                                      # a second game starts from the reset board and ends too
    if name == "zero":
        # every V ties: q = merge score << F, so boards where no move merges choose the smallest legal d
        flat = tr.boards.reshape(-1, 16)
        legal, acts = lg.legal_moves(flat), tr.action.reshape(-1)
        no_gain = tr.gain.reshape(-1) == 0
        assert (acts[no_gain] == np.argmax(legal[no_gain], axis=1)).all() and (no_gain & (acts > 0)).any()
    if name == "staged":
        stages = np.array([[sref.stage(b, THR_3) for b in row] for row in tr.boards[::20]])
        assert set(np.unique(stages)) == {0, 1, 2}                   # a board crosses both thresholds inside the run
    got = host_run(lib, case, tr.start, SEED, tr.t0 + 1, k)
    assert_same(got, want, name)


@pytest.mark.parametrize("T", [1, 4])
def test_other_tuple_counts(lib, T):
    """The networks above are T = 5 and 8; the smallest count and an even one, briefly (the GPU test plays every T)."""
    case, k = uniform_case(T), 40
    tr = trace_of(case, N, k, SEED)
    want = pref.limited(tr)
    assert pref.reaches(tr, want).directions == {0, 1, 2, 3} and want.episodes.sum() >= 1
    assert_same(host_run(lib, case, tr.start, SEED, tr.t0 + 1, k), want, f"T={T}")


@pytest.mark.parametrize("name", ["17x4", "staged"])
def test_budgets_follow_the_unlimited_trajectory_and_then_rest(lib, name):
    case, k, tr = run_of(name)
    left = budgets(N, 5)
    want = pref.limited(tr, left)
    hit = pref.reaches(tr, want)
    assert hit.ran_out and hit.never_moved and hit.two_episodes
    assert (want.games_left[left == 0] == 0).all() and (want.games_left[left == pref.NO_LIMIT] > 1 << 31).all()
    assert (want.games_left == 0).sum() > (left == 0).sum()          # a budget of 1 or 2 ran out inside the run
    got = host_run(lib, case, tr.start, SEED, tr.t0 + 1, k, games_left=left)
    assert_same(got, want, name)
    rest = left == 0
    assert np.array_equal(got.records[rest], tr.start[rest]) and (got.action[:, rest] == 0xff).all()
    assert int(got.hist.sum()) == int(left.astype(np.int64).sum() - got.games_left.astype(np.int64).sum()) == int(got.episodes.sum())


def test_engineered_boards(lib):
    case, k = uniform_case(), 12
    tr = engineered_trace(case, k)                                   # (shows what the boards reach)
    for games_left in (None, np.full(96, 2, np.uint32), budgets(96, 6)):
        want = pref.limited(tr, games_left)
        got = host_run(lib, case, tr.start, lg.SEED, tr.t0 + 1, k, games_left=games_left, board_offset=lg.BASE_OFFSET)
        assert_same(got, want, "engineered")


def test_max_tile_ends_episodes(lib):
    case, k = uniform_case(), 60
    tr = trace_of(case, N, k, SEED, max_exp=6)
    want = pref.limited(tr)
    ends = tr.terminal[tr.terminated] & 0x1f
    assert ((ends.max(axis=1) == 6) & (ends == 0).any(axis=1)).any()  # an episode ended on reaching 64 with cells to spare
    got = host_run(lib, case, tr.start, SEED, tr.t0 + 1, k, max_exp=6)
    assert_same(got, want, "max_tile")


def test_a_bad_description_is_refused(lib):
    case = uniform_case()
    bad = type(case.desc)(9, 4, 10, 1, 0)
    import ctypes as C
    assert lib.ntuple_play_check_run(None, 0, 0, 0, 0, 0, 0, C.byref(bad), *([None] * 10)) == -1
