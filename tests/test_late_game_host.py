"""CPU: the per-board step code of g2048_device.h (built for the host by tests/host_check) from the engineered late-game
boards of tests/late_game.py -- the last empty cell, full boards, terminal boards, max_tile, the deficit carry, 2^16 / 2^17
merges -- against the C oracle, and the proof that every family reaches what it names (its `check`, on the oracle alone).
tests/test_gpu_step_late_game.py then plays the same boards through every launch form on the device."""
import ctypes as C
import functools

import numpy as np
import pytest

import late_game as lg
from oracle import OracleBatch
from test_device_math_host import U8P, HostRecordBatch

FIELDS = ("boards", "score", "reward", "terminated", "illegal", "highest", "last_score", "last_len", "ep_count", "ep_start",
          "terminal_boards")
NAMES = ("rows", "one_hole", "full_a", "full_b", "carry", "high", "max_tile_2048", "max_tile_top")
FOLLOW_UP_STEPS = 11


@functools.lru_cache(maxsize=None)
def families():
    return {f.name: f for f in lg.all_families()}


def install(batch, fam):
    """late_game.install, and for a record batch the records: hostcheck_make_record of every board and score."""
    lg.install(batch, fam)
    if hasattr(batch, "records"):
        make = batch.hc.hostcheck_make_record
        for i in range(fam.n):
            make(batch.boards[i].ctypes.data_as(U8P), int(fam.scores[i]), batch.records[i].ctypes.data_as(U8P))
    return batch


class HostNumpyBatch(OracleBatch):
    """step_numpy_kernel's sequence on the host (hostcheck_step_batch_numpy: play_record_numpy + finish_record_numpy)."""

    def __init__(self, hc, n, seed=0, board_offset=0):
        super().__init__(n, seed, board_offset)
        self.hc = hc
        hc.hostcheck_step_batch_numpy.restype = None
        hc.hostcheck_step_batch_numpy.argtypes = self.lib.g2048o_step_batch_numpy.argtypes

    def step_numpy(self, actions=None, auto_reset=True):
        if actions is not None:
            actions = np.ascontiguousarray(actions, dtype=np.uint8)
        self.t += 1
        b = self._batch(actions)
        self.hc.hostcheck_step_batch_numpy(C.byref(b), self.rng.ctypes.data, self.n, self.seed, self.t, self.board_offset,
                                           self.illegal_move_reward, self.max_exp, int(auto_reset), 1)


def test_legal_moves_helper_matches_the_reference_table():
    """late_game.legal_moves picks the families' legal actions: it must be the reference's own legality."""
    from conftest import load_golden
    m = load_golden("move_table")
    assert np.array_equal(lg.legal_moves(m["boards"]), m["legal"].astype(bool))


@pytest.mark.parametrize("auto_reset", [True, False])
@pytest.mark.parametrize("unpacked", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_families_records_vs_oracle(host_check, name, unpacked, auto_reset):
    """One step from the engineered state with the family's actions (its check is asserted on the oracle's result), then --
    for every family but rows -- eleven more of the synthetic policy; every field after every step."""
    fam = families()[name]
    ora = install(OracleBatch(fam.n, lg.SEED, fam.offset), fam)
    host = install(HostRecordBatch(host_check, fam.n, lg.SEED, fam.offset, unpacked), fam)
    assert np.array_equal(host.records & 0x1F, fam.boards)
    for s in range(1 if name == "rows" else 1 + FOLLOW_UP_STEPS):
        for b in (ora, host):
            b.step(fam.actions if s == 0 else None, auto_reset=auto_reset)
        if s == 0:
            fam.check(ora)
        lg.check_scores(ora)
        for f in FIELDS:
            assert np.array_equal(getattr(ora, f), getattr(host, f)), (f, s)
        assert np.array_equal(host.records & 0x1F, ora.boards) and not (host.records[:, :8] & 0xE0).any(), s
        assert np.array_equal(lg.record_deficit(host.records), (lg.potential(ora.boards) - ora.score) % lg.SCORE_LIMIT), s


@pytest.mark.parametrize("auto_reset", [True, False])
@pytest.mark.parametrize("name", ["one_hole", "full_a", "full_b", "carry"])
def test_families_numpy_rng_mode_vs_oracle(host_check, name, auto_reset):
    """numpy-RNG mode: with one empty cell the reference's position draw is a choice among one, and an illegal move draws
    nothing -- the generator state after the step tells whether the host twin of the device code consumed what numpy does."""
    fam = families()[name]
    ora = OracleBatch(fam.n, lg.SEED, fam.offset)
    host = HostNumpyBatch(host_check, fam.n, lg.SEED, fam.offset)
    for b in (ora, host):
        b.seed_numpy(lg.SEED)
        install(b, fam)
    for s in range(1 + FOLLOW_UP_STEPS):
        for b in (ora, host):
            b.step_numpy(fam.actions if s == 0 else None, auto_reset=auto_reset)
        lg.check_scores(ora)
        for f in FIELDS + ("rng",):
            assert np.array_equal(getattr(ora, f), getattr(host, f)), (f, s)
    assert ora.terminated.any() or name == "carry"
