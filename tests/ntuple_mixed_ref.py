"""Reference of the mixed-length n-tuple network (include/g2048.h "mixed") -- TEST INFRASTRUCTURE ONLY.

The pure-Python references (ntuple_ref, ntuple_search_ref, ntuple_tc_ref, ntuple_trace_ref, ntuple_staged_ref) take cell
lists of any length per tuple and index ``weights[t, i]``; only the table width comes from ``len(tuples[0])``.  So the
reference of a mixed network is those modules, imported and not edited, on a PADDED array ``[S, T, 16^Lmax]`` in which
tuple t uses the first ``16^L_t`` entries of its row: ``mixed_net`` builds an ``ntuple_staged_ref.StagedNet`` on such an array
(S = 1, no thresholds, for a network of one weight set).  ``compact()`` / ``expand()`` move between the padded array and
the ``[S, W]`` layout of the definition and are written from it alone:

    base_t = sum over u < t of 16^L_u,   W = sum over t of 16^L_t,   element(stage, t, i) = stage * W + base_t + i

The shapes and boards the mixed tests share are here too.
"""
from __future__ import annotations

import numpy as np

import ntuple_ref as ref
import ntuple_staged_ref as sref
from ntuple_helpers import TUPLES_4x6, TUPLES_8x4

END = 0xff   # G2048_NTUPLE_END

MIX_ASC = ((5,), (0, 1), (4, 5, 6), (0, 1, 4, 5))                      # lengths 1..4: bases 0, 16, 272, 4368; W = 69 904
MIX_DESC = tuple(reversed(MIX_ASC))
MIX_8 = tuple(t[:n] for t, n in zip(TUPLES_8x4, (4, 1, 3, 2, 4, 2, 3, 1)))   # T at its limit
MIX_EXT = ((0, 1, 2, 3, 4, 5), (15,))                                  # the two extreme lengths, cell 15 in a list
PRESET = TUPLES_4x6 + ((0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 4, 5), (5, 6, 9, 10))   # "4x6+4x4"
SHAPES = {"asc": MIX_ASC, "desc": MIX_DESC, "8": MIX_8, "ext": MIX_EXT}


def lens(tuples):
    return [len(t) for t in tuples]


def bases(tuples):
    out, at = [], 0
    for n in lens(tuples):
        out.append(at)
        at += 16 ** n
    return out


def n_weights(tuples):
    return sum(16 ** n for n in lens(tuples))


def compact(padded, tuples):
    """[S, T, 16^Lmax] (or [T, 16^Lmax]) -> [S, W] (or [W]): the first 16^L_t entries of every row, back to back."""
    padded = np.asarray(padded)
    if padded.ndim == 2:
        return compact(padded[None], tuples)[0]
    out = np.zeros((padded.shape[0], n_weights(tuples)), padded.dtype)
    for t, (n, b) in enumerate(zip(lens(tuples), bases(tuples))):
        out[:, b:b + 16 ** n] = padded[:, t, :16 ** n]
    return out


def expand(flat, tuples, dtype=np.int64):
    """[S, W] (or [W]) -> [S, T, 16^Lmax] (or [T, 16^Lmax]), zero beyond each table."""
    flat = np.asarray(flat)
    if flat.ndim == 1:
        return expand(flat[None], tuples, dtype)[0]
    assert flat.shape[1] == n_weights(tuples)
    out = np.zeros((flat.shape[0], len(tuples), 16 ** max(lens(tuples))), dtype)
    for t, (n, b) in enumerate(zip(lens(tuples), bases(tuples))):
        out[:, t, :16 ** n] = flat[:, b:b + 16 ** n]
    return out


def mixed_net(tuples, thr=(), frac_bits=10, flat=None):
    """The reference network: a StagedNet (S = len(thr) + 1) on the padded array of ``flat`` ([S, W] int32 values)."""
    S = len(thr) + 1
    flat = np.zeros((S, n_weights(tuples)), np.int64) if flat is None else np.asarray(flat).reshape(S, -1)
    return sref.StagedNet(tuples, thr, frac_bits, expand(flat, tuples))


def random_flat(tuples, seed, S=1):
    """Full-range random int32 over the whole compact array: a look-up one element off reads another number."""
    return np.random.default_rng(seed).integers(-(1 << 31), 1 << 31, size=(S, n_weights(tuples))).astype(np.int32)


def flat_of(net):
    """[S, W] int64 of a reference network."""
    return compact(net.weights, net.tuples)


def tc_of(net, err=None, mag=None):
    """A StagedTC of ``net`` from compact accumulators ([S, W]; mag as the int64 bit pattern), zero when None."""
    tc = sref.StagedTC(net)
    if err is not None:
        tc.err[:] = expand(err, net.tuples)
        tc.mag[:] = expand(np.asarray(mag).view(np.int64), net.tuples).view(np.uint64)
    return tc


def tc_flat(tc, net):
    """(err, mag) [S, W] int64 bit patterns of a StagedTC."""
    return compact(tc.err, net.tuples), compact(tc.mag_i64(), net.tuples)


def lookups(board, net):
    """The compact elements (stage * W + base_t + idx) of the 8T look-ups of one board, in the order of ntuple_ref.value,
    from the definition and the reference's own trace."""
    b = ref.plain(board)
    hits = []
    ref.value(b, net.sub(0), hits)
    s, W, base = sref.stage(b, net.thr), n_weights(net.tuples), bases(net.tuples)
    return [s * W + base[t] + i for t, i in hits]


def table_edges(boards, net):
    """{(t, "first" | "last")}: the tables whose entry 0 / entry 16^L_t - 1 some board of ``boards`` reads."""
    out = set()
    for board in np.asarray(boards).reshape(-1, 16):
        hits = []
        ref.value(ref.plain(board), net.sub(0), hits)
        for t, i in hits:
            if i == 0:
                out.add((t, "first"))
            if i == 16 ** len(net.tuples[t]) - 1:
                out.add((t, "last"))
    return out


def all_edges(net):
    return {(t, e) for t in range(len(net.tuples)) for e in ("first", "last")}


def edge_boards():
    """[0]*16 reads entry 0 of every table; [15]*16 and [17]*16 (17 mod 32 clamps to 15) read the last."""
    return np.array([[0] * 16, [15] * 16, [17] * 16], np.uint8)


def cells_of(tuples, tuple_len=None):
    """uint8 [8, 6] cells of a descriptor, END-padded up to tuple_len (default: the longest list)."""
    L = max(lens(tuples)) if tuple_len is None else tuple_len
    out = np.zeros((8, 6), np.uint8)
    for t, cells in enumerate(tuples):
        out[t, :L] = END
        out[t, :len(cells)] = cells
    return out
