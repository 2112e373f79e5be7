"""CPU: restart_board of g2048_device.h -- the per-board body of restart_step_kernel and of the restart inside
ntuple_play_log_restart_kernel -- compiled for the host (tests/host_restart) and run in the kernel's lane structure, against the
sequential Python model (tests/restart_ref.py), bit for bit, on the engineered states of restart_ref.CASES: a position landing
on, one before and one after a stride multiple; q == C and q == C + 1 (the clamp); S' == S (no progress: a fresh board), by the
clamp and without it; R == min_span - 1 and R == min_span; restarts == max_restarts; pos == 2^32 - 1; k = 0 and k = 16; C = 1.
Every test first shows from the model alone that its cases are what their names say.  The same source file, built as a
stand-alone program under -fsanitize=address,undefined, is run directly.  All of it fails without the feature: the header has
no restart_board to compile."""
import subprocess

import numpy as np
import pytest

import restart_ref as rr
from restart_helpers import K_BLOCK, assert_state_equal, build_sanitized, host_restart_of, load_host_restart

RULES = list(rr.CASES)


@pytest.fixture(scope="module")
def lib():
    return load_host_restart()


def test_the_cases_are_what_their_names_say():
    ev = rr.expected_events(rr.BASE)
    assert (ev.restarts, ev.refused_span, ev.refused_max, ev.refused_progress, ev.clamped, ev.stores) == (8, 3, 1, 1, 3, 2)
    st, records, terminated = rr.case_state(rr.BASE, len(rr.CASES[rr.BASE]))
    names = [c[0] for c in rr.CASES[rr.BASE]]
    before = records.copy()
    snap = st.snap.copy()
    st.step(records, terminated)
    at = names.index

    def after(name):
        i = at(name)
        return int(st.pos[i]), int(st.start[i]), int(st.restarts[i])

    assert after("p one before a stride multiple") == (7, 0, 0) and after("p one after a stride multiple") == (9, 0, 0)
    i = at("p lands on a stride multiple")
    assert after("p lands on a stride multiple") == (8, 0, 0) and np.array_equal(st.snap[1, i], before[i])
    i = at("p lands on slot C")
    assert after("p lands on slot C") == (16, 4, 1) and np.array_equal(st.snap[3, i], before[i])
    assert after("p lands beyond slot C") == (20, 0, 0)
    assert after("pos at the end of its range") == (rr.U32, 0, 0) and after("pos one before the end") == (rr.U32, 0, 0)
    changed = {int(j) for j in np.argwhere((st.snap != snap).any(2))[:, 1]}
    assert changed == {at("p lands on a stride multiple"), at("p lands on slot C")}       # nothing else was stored
    for name, slot, want in (("restart from the middle", 1, (8, 8, 1)), ("restart, q == C", 3, (16, 16, 1)),
                             ("restart, q == C + 1 clamped", 3, (16, 16, 1)), ("restart of a restarted run", 3, (16, 16, 2)),
                             ("restarted run moves on", 2, (12, 12, 2)), ("R == min_span", 0, (4, 4, 1)),
                             ("restarts == max_restarts - 1", 3, (16, 16, 3)), ("pos at the end of its range, ended", 3, (16, 16, 1))):
        i = at(name)
        assert after(name) == want and np.array_equal(records[i], snap[slot, i]), name
    for name in ("S' == S by the clamp", "R == min_span - 1", "R == min_span - 1 in a restarted run", "restarts == max_restarts",
                 "fresh board ends at once"):
        i = at(name)
        assert after(name) == (0, 0, 0) and np.array_equal(records[i], before[i]), name
    # the other rules: k = 0, k = 16, C = 1, min_span below two strides and at 2^31 each restart and each refuse
    for rule in RULES[1:]:
        ev = rr.expected_events(rule)
        assert ev.restarts >= 1 and ev.refused_span + ev.refused_max + ev.refused_progress >= 1, rule
    assert {r.k for r in RULES} >= {0, 16} and 1 in {r.C for r in RULES}
    assert rr.expected_events(RULES[3]).refused_progress == 2               # S' == S without the clamp, and q == 0


@pytest.mark.parametrize("rule", RULES, ids=[f"k{r.k}-C{r.C}" for r in RULES])
@pytest.mark.parametrize("n, groups", [(None, 1), (64 * 3 + 5, 1), (2 * K_BLOCK + 77, 1), (2 * K_BLOCK + 77, 2)])
def test_restart_board_is_the_model(lib, rule, n, groups):
    """One board per case; a partial wave; a batch one workgroup strides over three times; two workgroups, a ragged last trip."""
    n = len(rr.CASES[rule]) if n is None else n
    want, records, terminated = rr.case_state(rule, n)
    got, got_records, _ = rr.case_state(rule, n)
    want.step(records, terminated)
    trips = lib.restart_check_step(got_records.ctypes.data, n, terminated.ctypes.data, host_restart_of(got), groups)
    assert trips == -(-n // (groups * K_BLOCK))
    assert np.array_equal(got_records, records), f"records differ at boards {np.argwhere((got_records != records).any(1))[:4, 0].tolist()}"
    assert_state_equal(got, want, f"{rule} n={n}")


def test_three_steps_in_a_row(lib):
    """The state a step leaves is the state the next one finds: the restarted boards run on and store again."""
    rule, n = rr.BASE, 61
    want, records, terminated = rr.case_state(rule, n)
    got, got_records, _ = rr.case_state(rule, n)
    rng = np.random.default_rng(5)
    for step in range(3):
        want.step(records, terminated)
        assert lib.restart_check_step(got_records.ctypes.data, n, terminated.ctypes.data, host_restart_of(got), 1) == 1
        assert np.array_equal(got_records, records)
        assert_state_equal(got, want, f"step {step}")
        terminated = (rng.random(n) < 0.3).astype(np.uint8)
        records[:] = got_records[:] = rng.integers(0, 256, (n, 16)).astype(np.uint8)
    assert want.events.restarts > 8 and want.events.stores > 2


def test_bad_arguments_are_refused(lib):
    import ctypes as C
    from restart_helpers import HostRestart
    st, records, terminated = rr.case_state(rr.BASE, 4)
    ok = host_restart_of(st)
    assert lib.restart_check_step(records.ctypes.data, 4, terminated.ctypes.data, C.byref(ok), 0) == -1
    assert lib.restart_check_step(None, 4, terminated.ctypes.data, C.byref(ok), 1) == -1
    for field, value in (("stride_log2", 17), ("capacity", 0), ("capacity", 4097), ("min_span", 1), ("min_span", (1 << 31) + 1),
                         ("max_restarts", 0), ("snap", None)):
        bad = HostRestart.from_buffer_copy(ok)
        setattr(bad, field, value)
        assert lib.restart_check_step(records.ctypes.data, 4, terminated.ctypes.data, C.byref(bad), 1) == -1, field


def test_the_stand_alone_program_runs_clean_under_the_sanitizers():
    """restart_check.cpp with its own main, -fsanitize=address,undefined, run directly (not loaded into Python): random states of
    every stride and capacity edge against a second model, no report from either sanitizer."""
    out = subprocess.run([build_sanitized()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "restart_check ok" in out.stdout and "Sanitizer" not in out.stderr and "runtime error" not in out.stderr
