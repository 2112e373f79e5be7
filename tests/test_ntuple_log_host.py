"""CPU: ntuple_play_log_step and ntuple_log_delta of g2048_device.h -- the per-board bodies of ntuple_play_log_kernel and
ntuple_log_delta_kernel -- compiled for the host (tests/host_ntuple_log) and run in the kernels' lane structure, against the
pure-Python reference (tests/ntuple_log_ref.py: ntuple_td_helpers.reference_steps kept in a log, the delta rule of
include/g2048.h, the existing update references).  Bit for bit: after, gain and flag of every slot after each of two
consecutive calls (the second shows the carry of slot M into slot 0), the records with their score-deficit bits, the terminal
records, the episode and illegal-end counts and the gain sum; delta of every slot under the log's own flags and under flags
overwritten with all 256 byte values.  Every test first shows from the reference alone that its run reaches what it names.
The tests that take ``lib`` fail without the feature: the header has nothing to compile.  Three do not and pass without it,
because they look at the reference alone -- test_the_start_boards_are_what_the_issue_counts (the issue's table of start boards)
and both cases of test_the_reference_sweep_changes_every_table_and_depends_on_the_order (the sweep of the reference against
itself: order, TD against TC): they are the guards the other tests and the GPU tests stand on."""
import numpy as np
import pytest

import ntuple_log_ref as lref
import ntuple_ref as ref
import ntuple_tc_ref as tcref
from ntuple_log_helpers import K_BLOCK, all_flag_bytes, assert_log_case, host_delta, host_play_rounds, load_host_log
from ntuple_td_helpers import CASES, small_case, uniform_case

ROUNDS = 2


@pytest.fixture(scope="module")
def lib():
    return load_host_log()


def assert_play_equal(got, want, logs, n, M, where):
    assert got.lanes == [-(-n // K_BLOCK) * K_BLOCK] * ROUNDS
    for r in range(ROUNDS):
        lref.assert_logs_equal(got.logs[r], logs[r], f"{where}, call {r}")
    assert np.array_equal(got.records, want.steps[-1].records), f"{where}: records"
    assert np.array_equal(got.last_records, want.last_records), f"{where}: last_records"
    for name in ("episodes", "illegal_ends", "gain_sum"):
        assert getattr(got, name) == getattr(want, name), f"{where}: {name}"


# ------------------------------------------------------------------------------------------------ the guards of the issue's table
def test_the_start_boards_are_what_the_issue_counts():
    """n = 1: 3 moves, its only board has no legal move, [1, 0, 0] episodes end; n = 65: 6 moves, 13 boards without a legal move
    at the first move, 21|3|3|4|2|2 ("small") and 19|3|5|5|6|2 ("17x4") episodes end per move, at least 350 live entries."""
    want, logs = lref.frozen_rounds(small_case(), 1, 3, 1)
    assert want.no_move[0, 0] and [int(s.terminated.sum()) for s in want.steps] == [1, 0, 0]
    assert int((logs[0].flag != 0).sum()) == 2
    for case, ended in ((small_case(), [21, 3, 3, 4, 2, 2]), (uniform_case(), [19, 3, 5, 5, 6, 2])):
        want, logs = lref.frozen_rounds(case, 65, 6, 1)
        assert int(want.no_move[0].sum()) == 13
        assert [int(s.terminated.sum()) for s in want.steps] == ended
        assert int((logs[0].flag != 0).sum()) >= 350
    # n = 257: 6 moves, 26 boards without a legal move at the first move, at least 3 episodes end at every move, at least 1 462 live entries
    for case in (small_case(), uniform_case()):
        want, logs = lref.frozen_rounds(case, 257, 6, ROUNDS)
        assert int(want.no_move[0].sum()) == 26
        assert all(int(s.terminated.sum()) >= 3 for s in want.steps[:6])
        assert int((logs[0].flag != 0).sum()) >= 1462


# ------------------------------------------------------------------------------------------------ play_log
PLAY_CASES = [(name, n, M) for name in sorted(CASES) for n, M in ((1, 3), (3, 1), (65, 2), (65, 6))] + [("small", 257, 6)]


@pytest.mark.parametrize("name, n, M", PLAY_CASES, ids=[f"{name}-n{n}-M{M}" for name, n, M in PLAY_CASES])
def test_play_log_is_the_reference(lib, name, n, M):
    case = CASES[name]()
    want, logs = lref.frozen_rounds(case, n, M, ROUNDS)
    if n >= 65:
        assert_log_case(logs, n, M)
    else:
        r = lref.reaches(logs)
        assert r.empty_slot0 and logs[0].flag[1, 0] == 0             # board 0 has no legal move at the first move
        assert np.array_equal(logs[1].flag[0], logs[0].flag[M]) and np.array_equal(logs[1].after[0], logs[0].after[M])
    got = host_play_rounds(lib, case, want.start, M, ROUNDS)
    assert_play_equal(got, want, logs, n, M, f"{name} n={n} M={M}")


def test_one_call_of_six_moves_is_six_calls_of_one(lib):
    """Slot m of one M = 6 call is slot 1 of the m-th M = 1 call (whose slot 0 is the slot 1 of the call before it), and the
    records, terminal records and counts agree."""
    case = small_case()
    want, _ = lref.frozen_rounds(case, 65, 6, 1)
    six, ones = host_play_rounds(lib, case, want.start, 6, 1), host_play_rounds(lib, case, want.start, 1, 6)
    for m in range(1, 7):
        for name in ("after", "gain", "flag"):
            assert np.array_equal(getattr(ones.logs[m - 1], name)[1], getattr(six.logs[0], name)[m]), f"slot {m}: {name}"
            assert np.array_equal(getattr(ones.logs[m - 1], name)[0], getattr(six.logs[0], name)[m - 1]), f"slot {m}: carried {name}"
    assert np.array_equal(six.records, ones.records) and np.array_equal(six.last_records, ones.last_records)
    assert (six.episodes, six.illegal_ends, six.gain_sum) == (ones.episodes, ones.illegal_ends, ones.gain_sum)


def test_max_tile_ends_episodes(lib):
    case = uniform_case()
    want, logs = lref.frozen_rounds(case, 256, 3, ROUNDS, max_exp=7)
    plain, _ = lref.frozen_rounds(case, 256, 3, ROUNDS)
    assert want.episodes > plain.episodes                            # the limit ended episodes that run on without it
    got = host_play_rounds(lib, case, want.start, 3, ROUNDS, max_exp=7)
    assert_play_equal(got, want, logs, 256, 3, "max_tile")


# ------------------------------------------------------------------------------------------------ log_delta
@pytest.mark.parametrize("name", sorted(CASES))
def test_log_delta_is_the_reference(lib, name):
    case = CASES[name]()
    n, M = 65, 6
    _, logs = lref.frozen_rounds(case, n, M, ROUNDS)
    assert_log_case(logs, n, M)
    for r, log in enumerate(logs):
        nonzero = 0
        for m in range(M):
            want = lref.log_delta(case.rnet, log, m)
            got, evals, lanes = host_delta(lib, case, log, m)
            assert lanes == K_BLOCK
            assert np.array_equal(got, want), f"{name} call {r} slot {m}: boards {np.argwhere(got != want)[:4, 0].tolist()}"
            f, f1 = log.flag[m].astype(int), log.flag[m + 1].astype(int)
            self_read = ((f & 1) != 0) & (((f & 2) != 0) | ((f1 & 1) != 0))
            next_read = ((f & 1) != 0) & ((f & 2) == 0) & ((f1 & 1) != 0)
            assert evals == int(self_read.sum()) + int(next_read.sum())   # what the rule does not read is not evaluated
            nonzero += int((want != 0).sum())
        assert nonzero >= 100


def test_log_delta_is_total_for_any_flag_byte(lib):
    case = small_case()
    n, M = 65, 6
    _, logs = lref.frozen_rounds(case, n, M, ROUNDS)
    flag = all_flag_bytes(M, n)
    assert set(np.unique(flag).tolist()) == set(range(256))
    pairs = {(int(a) & 3, int(b) & 3) for a, b in zip(flag[:-1].reshape(-1), flag[1:].reshape(-1))}
    assert len(pairs) == 16                                            # every combination of the two bits read, in both bytes
    for m in range(M):
        want = lref.log_delta(case.rnet, logs[1], m, flag=flag)
        got, _, _ = host_delta(lib, case, logs[1], m, flag=flag)
        assert np.array_equal(got, want), f"slot {m}"
        low = lref.log_delta(case.rnet, logs[1], m, flag=flag & 3)
        assert np.array_equal(want, low)                                # only bits 0 and 1 are read


def test_bad_arguments_are_refused(lib):
    import ctypes as C
    from ntuple_log_helpers import HostLog, host_log_of
    case = uniform_case()
    log = lref.Log(4, 2)
    h = host_log_of(log)
    delta = np.zeros(4, np.int64)
    assert lib.log_check_delta(4, C.byref(case.desc), case.w32.ctypes.data, C.byref(h), 2, delta.ctypes.data, None) == -1   # m >= M
    assert lib.log_check_delta(4, C.byref(case.desc), case.w32.ctypes.data, C.byref(HostLog(0, 1, 1, 1)), 0, delta.ctypes.data, None) == -1
    bad = type(case.desc)(9, 4, 10, 1, 0)
    assert lib.log_check_delta(4, C.byref(bad), None, C.byref(h), 0, delta.ctypes.data, None) == -1
    assert lib.log_check_play(None, 4, 0, 0, 0, 0, C.byref(bad), None, C.byref(h), None, None) == -1


# ------------------------------------------------------------------------------------------------ the reference's sweep, by itself
def sweep_results(case, n, M, lr_shift):
    """(start, TD, TC, ascending-order TD) weights of one sweep over the first round's reference log."""
    _, logs = lref.frozen_rounds(case, n, M, 1)
    out = {}
    for key, kw in (("td", {}), ("tc", {"tc": True}), ("up", {"order": range(M)})):
        net = case.rnet.copy()
        tc = tcref.TC(net) if kw.pop("tc", False) else None
        lref.sweep(net, logs[0], lr_shift, tc=tc, **kw)
        out[key] = net.weights
    return case.rnet.weights, out


@pytest.mark.parametrize("name, lr_shift", [("small", 2), ("17x4", 8)])
def test_the_reference_sweep_changes_every_table_and_depends_on_the_order(name, lr_shift):
    case = CASES[name]()
    assert isinstance(case.rnet, ref.Net)
    start, out = sweep_results(case, 65, 6, lr_shift)
    for t in range(len(case.tuples)):
        assert not np.array_equal(out["td"][t], start[t]), f"table {t} does not change"
    assert not np.array_equal(out["tc"], out["td"]), "the TC result differs from the TD result"
    assert not np.array_equal(out["up"], out["td"]), "sweeping in ascending m gives other weights"
