"""Shared by the n-tuple expectimax tests: the boards the tests use and the comparison of two search results (the host build
is ntuple_helpers').  A plain module, like ntuple_helpers."""
import numpy as np

SEARCH_NAMES = ("action", "value")
SEARCH_GROUP = {1: 16, 2: 64}   # kNtupleSearchGroup<D> (g2048_kernels.hip): lanes per board at depth D

# a full board whose only legal moves are left and right (the pair of 1s in the first row); either leaves one empty cell, a
# corner, and the board with a 2 there (exponent 1) has no move while the board with a 4 (exponent 2) can merge it
PAIR_ONLY = np.array([[1, 1, 3, 2, 5, 6, 7, 4, 1, 2, 3, 5, 4, 5, 6, 7]], np.uint8)


def _sparse(cells, exponents):
    b = np.zeros(16, np.uint8)
    b[list(cells)] = exponents
    return b


# Boards whose afterstates have E = 15, 14, 12, 9, 8 and 7 empty cells: 30, 28, 24, 18, 16 and 14 chance items in a
# direction.  On the 16 lanes a direction has at depth 2, 16 items are one full pass, 18 a second pass on two lanes, 24
# on eight, 30 on all but two (tests assert the counts from the reference's trace).  One- and two-tile boards give E = 15.
WIDE_FANS = np.array([
    _sparse([5], [3]), _sparse([0], [1]), _sparse([0, 1], [1, 1]), _sparse([6, 9], [2, 5]),
    _sparse([0, 2, 5, 7], [1, 2, 1, 2]), _sparse([0, 5, 10, 15], [3, 1, 2, 4]),
    _sparse(range(7), [1, 2, 3, 4, 2, 3, 1]), _sparse(range(8), [1, 2, 3, 4, 2, 3, 4, 5]),
    _sparse(range(9), [1, 2, 3, 4, 2, 3, 4, 5, 1]), _sparse([0, 2, 5, 7, 8, 10, 13], [1, 2, 3, 1, 2, 3, 1])], np.uint8)


def assert_search_equal(got, want, boards=None, where=""):
    for name, g, w in zip(SEARCH_NAMES, got, want):
        g, w = np.asarray(g), np.asarray(w)
        bad = np.nonzero((g.reshape(len(g), -1) != w.reshape(len(w), -1)).any(1))[0]
        assert len(bad) == 0, (f"{where}: {name} differs on {len(bad)} boards, first row {bad[0]}"
                               f"{'' if boards is None else ' ' + str(np.asarray(boards).reshape(-1, 16)[bad[0]].tolist())}: "
                               f"{g[bad[0]].tolist()} vs {w[bad[0]].tolist()}")
