"""Shared by the temporal-coherence tests: accumulators pre-loaded so that a batch reaches the edges of the rate, deltas, and
the comparison of the three tables (the host build is ntuple_helpers').  A plain module, like ntuple_helpers."""
import numpy as np

import ntuple_tc_ref as tcref


# (E, A) pairs that reach every branch of the rate: never updated; E = 0; |E| = A; |E| = A - 1; A at and around 2^32, 2^63
# and 2^64 - 1 (k > 0); |E| > A (not reachable by updates, defined all the same); E = INT64_MIN
EDGE_PAIRS = [(0, 0), (5, 0), (0, 7), (9, 9), (-9, 9), (8, 9), (-1, 1 << 20), (1 << 31, (1 << 32) - 1), (-(1 << 31), 1 << 32),
              ((1 << 32), (1 << 32) + 1), (-(1 << 62), 1 << 63), ((1 << 63) - 1, (1 << 64) - 1), (-(1 << 63), (1 << 64) - 1),
              (10, 3), (-(1 << 40), 1 << 33), (-(1 << 63), 5), (-(1 << 63), 1 << 63), (1, (1 << 64) - 1), (3, 1 << 17)]


def preload(net, seed, boards=None):
    """A reference TC for ``net`` whose accumulators are random with bitlen(A) uniform in 0..64 and |E| <= A; the entries
    the ``boards`` reach cycle through EDGE_PAIRS so that a small batch meets every edge."""
    rng = np.random.default_rng(seed)
    shape = net.weights.shape
    bits = rng.integers(0, 65, size=shape)
    top = rng.integers(0, 1 << 64, size=shape, dtype=np.uint64) | np.uint64(1 << 63)
    mag = top >> (64 - np.maximum(bits, 1)).astype(np.uint64)       # bitlen(mag) == bits
    mag[bits == 0] = 0
    half = mag >> np.uint64(1)
    kind = rng.integers(0, 4, size=shape)                           # |E| = A (where it fits), E = 0, or somewhere below A / 2
    mask = rng.integers(0, 1 << 64, size=shape, dtype=np.uint64)
    err = np.where(kind == 0, np.where(bits < 64, mag, half), np.where(kind == 1, np.uint64(0), half & mask)).astype(np.int64)
    err = err * rng.choice(np.array([-1, 1], np.int64), size=shape)
    tc = tcref.TC(net, err.astype(np.int64), mag)
    if boards is not None:
        k = 0
        for b in np.asarray(boards).reshape(-1, 16):
            for t, i in tcref.hits_of(b, net):
                e, a = EDGE_PAIRS[k % len(EDGE_PAIRS)]
                tc.err[t, i], tc.mag[t, i] = e, a
                k += 1
    return tc


def edge_deltas(n, seed):
    """Mixed-sign deltas of every size up to beyond the clamp, with zeros."""
    rng = np.random.default_rng(seed)
    d = rng.integers(-(1 << 20), 1 << 20, n) << rng.integers(0, 24, n)
    d[::9] = 0
    special = [(1 << 40) + 1, -(1 << 40) - 1, tcref.INT64_MAX, tcref.INT64_MIN, 1 << 40, -(1 << 40), 1, -1, 1 << 31, -(1 << 31) - 1]
    d[1::13][:len(special)] = special[:len(d[1::13])]
    return d


def assert_tables_equal(got, want, names=("weights", "err", "mag")):
    for name, g, w in zip(names, got, want):
        g, w = np.asarray(g), np.asarray(w)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, f"{len(bad)} entries of {name} differ, first {bad[0].tolist()}: {g[tuple(bad[0])]} vs {w[tuple(bad[0])]}"
