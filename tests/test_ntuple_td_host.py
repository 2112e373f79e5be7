"""CPU: ntuple_td_step of g2048_device.h -- the per-board body of ntuple_td_step_kernel -- compiled for the host
(tests/host_ntuple_td) and run in the kernel's lane structure, against the same step composed by hand of ntuple_root,
ntuple_play_step and reset_record in the same build, and against the reference model: the oracle's step under the pure-Python
references' evaluate (ntuple_td_helpers.reference_steps).  Bit for bit: the six outputs of every step, the records with their
score-deficit bits, the terminal records, the episode and illegal-end counts and the gain sum.  Every test first shows from
the reference's own trace (never from the code under test) that its run reaches what it names.  These tests fail without the
feature: the header has no ntuple_td_step to compile."""
import numpy as np
import pytest

from ntuple_td_helpers import CASES, K_BLOCK, assert_same_steps, host_steps, load_host_td, reference_steps, uniform_case

K = 6           # consecutive steps: the boards that ended an episode in step 0 are evaluated as fresh boards and play on


@pytest.fixture(scope="module")
def lib():
    return load_host_td()


def assert_reaches(want, n):
    """From the reference alone: what a run of n boards is there for."""
    first = want.steps[0]
    assert want.no_move[0, 0] and first.terminated[0] == 1 and first.action[0] == 0 and first.after_value[0] == 0  # no legal move
    assert np.array_equal(first.after[0], want.start[0] & 0x1f) and first.delta[0] == 0
    assert want.episodes >= 1 and want.illegal_ends >= 1
    if n >= 64:
        ended = np.array([s.terminated for s in want.steps], bool)
        assert (ended & ~want.no_move).any(), "an episode ends on a legal move"
        assert (~ended).any() and int(want.no_move.sum()) >= 12
        assert want.illegal_ends < want.episodes
        q = np.array([s.after_value for s in want.steps])
        assert (q < 0).any() and (np.array([s.delta for s in want.steps]) != 0).any()
        assert {int(a) for s in want.steps for a in s.action} == {0, 1, 2, 3}
        # a board that ended in step j is a fresh board in step j + 1: two tiles, and it moves
        after_end = ended[:-1] & ~want.no_move[1:]
        assert after_end.any()


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("n", [1, 3, 64, 256])
def test_fused_body_is_the_composition_and_the_reference(lib, name, n):
    case = CASES[name]()
    want = reference_steps(case, n, K)
    assert_reaches(want, n)
    fused = host_steps(lib, "fused", case, want.start, K)
    assert fused.lanes == [-(-n // K_BLOCK) * K_BLOCK] * K         # whole blocks: n = 1, 3 and 64 run 255, 253 and 192 lanes past the end
    composed = host_steps(lib, "composed", case, want.start, K)
    assert composed.lanes == [n] * K                                # (and ntuple_play_step played the first root's action)
    assert_same_steps(fused, composed, f"{name} n={n}: fused vs composed")
    assert_same_steps(fused, want, f"{name} n={n}: fused vs reference")


def test_ties_choose_the_smallest_direction(lib):
    """Under the small signed weights two directions tie on q somewhere in the run (shown from the reference's q), and the
    fused body takes the smaller one."""
    import ntuple_ref as ref
    case = CASES["small"]()
    want = reference_steps(case, 256, K)
    ties = 0
    for j, s in enumerate(want.steps):
        boards = (want.start if j == 0 else want.steps[j - 1].records) & 0x1f
        q = ref.evaluate_batch(boards, case.rnet)[0]
        legal = q != ref.ILLEGAL
        top = np.where(legal, q, np.iinfo(np.int64).min).max(axis=1)
        tied = ((q == top[:, None]) & legal).sum(axis=1) >= 2
        ties += int(tied.sum())
        assert (s.action[tied] == np.argmax((q == top[:, None]) & legal, axis=1)[tied]).all()
    assert ties >= 1
    assert_same_steps(host_steps(lib, "fused", case, want.start, K), want, "small: ties")


def test_max_tile_ends_episodes(lib):
    case = uniform_case()
    want = reference_steps(case, 256, K, max_exp=7)
    ended = np.array([s.terminated for s in want.steps], bool)
    assert (ended & ~want.no_move).any()
    fused = host_steps(lib, "fused", case, want.start, K, max_exp=7)
    assert_same_steps(fused, want, "max_tile")
    assert_same_steps(fused, host_steps(lib, "composed", case, want.start, K, max_exp=7), "max_tile: fused vs composed")
    assert want.episodes > reference_steps(case, 256, K).episodes   # the limit ended episodes that run on without it


def test_a_bad_description_is_refused(lib):
    import ctypes as C
    case = uniform_case()
    bad = type(case.desc)(9, 4, 10, 1, 0)
    for fn in (lib.td_check_fused, lib.td_check_composed):
        assert fn(None, 4, 0, 0, 0, 0, C.byref(bad), None, None) == -1
