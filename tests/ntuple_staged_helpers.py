"""Shared by the multi-stage n-tuple tests: the low thresholds that let small boards populate every stage, and the boards
the tests use (the host build is ntuple_helpers').  A plain module, like ntuple_helpers."""
import numpy as np

import ntuple_staged_ref as sref
from analysis_helpers import mixed_boards

# "has a 4", "has an 8", "has a 16 and an 8": S = 4, and a spawned 4 alone crosses the first threshold
LOW_THR = (sref.stage_mask(4), sref.stage_mask(8), sref.stage_mask(16, 8))
# S = 8 on small boards
THR_8 = (4, 8, 12, 16, 24, 32, 48)


# ------------------------------------------------------------------------------------------------ boards
def small_boards(n, seed, max_exp=None):
    """Random boards at mixed densities whose largest exponent cycles through 1..5 from board to board (or is ``max_exp``),
    every sixth one a board of the golden trajectories: small tiles, so the low thresholds above put boards into every
    stage, and many boards have a move or a spawn that makes the tile a threshold asks for."""
    rng = np.random.default_rng(seed)
    density = rng.uniform(0.2, 1.0, size=(n, 1))
    top = np.full((n, 1), max_exp) if max_exp else np.arange(n).reshape(n, 1) % 5 + 1
    b = np.where(rng.random((n, 16)) < density, rng.integers(0, 1 << 16, size=(n, 16)) % top + 1, 0).astype(np.uint8)
    b[5::6] = mixed_boards(n, seed)[::2][:len(b[5::6])]
    return b


def depth2_boards(boards, full=3):
    """Boards a pure-Python depth-2 search can afford: the ``full`` boards with the fewest empty cells, and one board of two
    2s whose move merges nothing -- its afterstate holds no 4, so a spawned 4 alone crosses stage_mask(4) below it."""
    boards = np.asarray(boards, np.uint8).reshape(-1, 16)
    two = np.zeros((1, 16), np.uint8)
    two[0, [0, 5]] = 1
    return np.concatenate([boards[np.argsort((boards == 0).sum(1), kind="stable")[:full]], two])


def sparse_boards(k, seed, empties=(5, 8)):
    """k boards of small_boards with 5..8 empty cells: chance nodes of 10..16 items, so the lanes of a depth-2 search that
    split a chance node (items sub, sub + K, ...) each get several."""
    pool = small_boards(25 * k, seed)
    e = (pool == 0).sum(1)
    out = pool[(e >= empties[0]) & (e <= empties[1])][:k]
    assert len(out) == k
    return out


# one 4-tuple (the corner square): the network that keeps the pure-Python depth-2 search of sparse boards affordable
ONE_TUPLE = ((0, 1, 4, 5),)


def with_deficit_bits(boards, seed):
    """Engine-record bytes of plain boards: random score-deficit bits in bits 5..7 of bytes 8..15."""
    raw = np.array(boards, np.uint8).reshape(-1, 16) & 0x1f
    raw[:, 8:] |= (np.random.default_rng(seed).integers(0, 8, size=raw[:, 8:].shape) << 5).astype(np.uint8)
    return raw


def preload_tc(net, seed):
    """A StagedTC with small random accumulators everywhere: rates between 0 and 1 on every look-up."""
    rng = np.random.default_rng(seed)
    mag = rng.integers(0, 1 << 20, size=net.weights.shape).astype(np.uint64)
    err = (rng.integers(-(1 << 20), 1 << 20, size=net.weights.shape) % (mag.astype(np.int64) + 1)).astype(np.int64)
    return sref.StagedTC(None, err, mag)
