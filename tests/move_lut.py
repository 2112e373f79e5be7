"""The oracle's shift() as a row table -- TEST INFRASTRUCTURE ONLY: afterstates, merge scores and legality masks of plain
boards (exponents < 18) without any device code, shared by the afterstate, search and large-output tests and the fuzz."""
import ctypes as C

import numpy as np

from conftest import load_golden


def row_index(rows):
    r = rows.astype(np.int64)
    return ((r[..., 0] * 18 + r[..., 1]) * 18 + r[..., 2]) * 18 + r[..., 3]


_cache = {}


def build_row_lut(oracle_lib):
    """shift() of every row of exponents 0..17 (the meshgrid order of shift_exhaustive), from the oracle's g2048o_shift,
    pinned against the fixture captured from the reference.  (out uint8 [18^4, 4], score int32 [18^4]); built once."""
    if "lut" in _cache:
        return _cache["lut"]
    rows = np.array(np.meshgrid(*[np.arange(18)] * 4, indexing="ij")).reshape(4, -1).T.astype(np.uint8)
    out = np.empty_like(rows)
    score = np.empty(len(rows), np.int32)
    vin, vout = (C.c_int64 * 4)(), (C.c_int64 * 4)()
    for k, row in enumerate(rows):
        for j in range(4):
            vin[j] = (1 << int(row[j])) if row[j] else 0
        score[k] = oracle_lib.g2048o_shift(vin, vout)
        out[k] = [int(v).bit_length() - 1 if v else 0 for v in vout]
    g = load_golden("shift_exhaustive")
    assert np.array_equal(row_index(rows), np.arange(len(rows)))
    assert np.array_equal(out, g["out"]) and np.array_equal(score, g["score"])
    _cache["lut"] = (out, score)
    return out, score


def lut_afterstates(boards, lut):
    """(new [n,4,16], score [n,4], legal mask [n]) of plain boards (exponents < 18) through the row table."""
    out_lut, score_lut = lut
    b = np.asarray(boards, np.uint8).reshape(-1, 4, 4)
    assert b.max() < 18
    n = len(b)

    def left(x):
        idx = row_index(x)
        return out_lut[idx], score_lut[idx].sum(axis=1)

    new = np.empty((n, 4, 16), np.uint8)
    score = np.empty((n, 4), np.int32)
    t = lambda x: x.transpose(0, 2, 1)            # noqa: E731
    r = lambda x: x[:, :, ::-1]                   # noqa: E731
    v = lambda x: x[:, ::-1, :]                   # noqa: E731
    o, s = left(t(b)); new[:, 0], score[:, 0] = t(o).reshape(n, 16), s               # up
    o, s = left(r(b)); new[:, 1], score[:, 1] = r(o).reshape(n, 16), s               # right
    o, s = left(t(v(b))); new[:, 2], score[:, 2] = v(t(o)).reshape(n, 16), s         # down
    o, s = left(b); new[:, 3], score[:, 3] = o.reshape(n, 16), s                     # left
    changed = (new != b.reshape(n, 1, 16)).any(axis=2)
    mask = (changed.astype(np.uint8) << np.arange(4, dtype=np.uint8)).sum(axis=1).astype(np.uint8)
    return new, score, mask


def onehot_ref(boards, dtype):
    """stack() (game2048_env.py:17-32) by F.one_hot: uint8 exponents [..., 16] (a device tensor) -> [..., 16, 4, 4] of
    ``dtype``; channel c = (exponent == c) for c < 16, so an exponent of 16..31 sets no channel.  The range is checked
    first: an index outside num_classes is a device-side assert in one_hot, not an exception."""
    import torch.nn.functional as F
    b = boards.long()
    assert b.numel() == 0 or int(b.max()) < 32
    return F.one_hot(b, 32)[..., :16].transpose(-1, -2).reshape(b.shape[:-1] + (16, 4, 4)).to(dtype)
