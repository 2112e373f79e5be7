"""Test helper: the episode slots and the terminal records inside a ``Batched2048.state_dict()`` blob.

The blob is the 56-byte ``StateHeader`` followed by the game region of the engine's slab (g2048_create): board records,
terminal records, the episode slots, the statistics struct, the returns-summary scratch and the graph clock word, each
region starting on a 256-byte boundary (the last three are the engine's work memory: zeros in a blob, ignored on load);
in numpy-RNG mode the five generator planes (40 bytes per board) follow.  A slot holds
four 64-bit counters of 64 boards as eight dwords, the four low halves first: {episodes, illegal_ends, G, pending}.
There are slots for whole 512-lane blocks (the block of step_numpy_kernel), so a batch that is not a multiple of 512
has padding slots behind the ``n_waves`` ones the readers sum.

``StateBlob`` checks the size it computes against the blob it is given, so that a change of the layout fails here
instead of planting counters in the wrong place; ``check_slots_match_stats`` checks the slot offset against what the
engine itself reports.
"""
from __future__ import annotations

import numpy as np

HEADER_BYTES = 56           # StateHeader: 5 x u64, i32, u32, f32, u32
SLOT_DWORDS = 8
SLOT_BLOCK_LANES = 512      # kSlotBlockLanes
STATS_BYTES = 176           # g2048_stats
SUMMARY_SCRATCH_BYTES = 2048 * 8
EP, ILL, GAIN, PEND = 0, 1, 2, 3


def _up(x: int) -> int:
    return (x + 255) & ~255


def n_waves(n: int) -> int:
    """Slots the statistics readers sum: one per 64 boards."""
    return (n + 63) // 64


def n_slots(n: int) -> int:
    """Slots the engine allocates: whole 512-lane blocks."""
    return (n + SLOT_BLOCK_LANES - 1) // SLOT_BLOCK_LANES * (SLOT_BLOCK_LANES // 64)


def slab_offsets(n: int) -> dict:
    """Byte offsets of the regions inside the blob's game region (not counting the header) and its size."""
    records = 0
    last = records + _up(16 * n)
    slots = last + _up(16 * n)
    stats = slots + _up(n_slots(n) * SLOT_DWORDS * 4)
    summary = stats + _up(STATS_BYTES)
    graph_t = summary + _up(SUMMARY_SCRATCH_BYTES)
    return dict(records=records, last_records=last, slots=slots, slab_bytes=graph_t + 256)


class StateBlob:
    """A private copy of an engine's state blob with writable views of its slots and terminal records."""

    def __init__(self, eng, state=None):
        self.n = n = eng.n_envs
        if state is None:
            self.state = eng.state_dict()
            self.blob = self.state["blob"]          # (a blob of its own: no second copy of a large slab)
        else:
            self.state = state
            self.blob = np.ascontiguousarray(state["blob"]).copy()
        off = slab_offsets(n)
        rng_bytes = 40 * n if self.state.get("rng_mode") == "numpy" else 0
        assert self.blob.size == HEADER_BYTES + off["slab_bytes"] + rng_bytes, \
            f"state blob of {self.blob.size} bytes: the slab layout this helper assumes has changed"
        assert int(self.blob[:HEADER_BYTES].view(np.uint64)[1]) == n, "StateHeader.n"
        base = HEADER_BYTES
        s = base + off["slots"]
        self.slots = self.blob[s: s + n_slots(n) * SLOT_DWORDS * 4].view(np.uint32).reshape(-1, SLOT_DWORDS)
        r = base + off["last_records"]
        self.last_records = self.blob[r: r + 16 * n].reshape(n, 16)
        b = base + off["records"]
        self.records = self.blob[b: b + 16 * n].reshape(n, 16)

    def counters(self) -> np.ndarray:
        """uint64 [n_slots, 4]: the slots' 64-bit counters (low dword | high dword << 32)."""
        lo = self.slots[:, 0:4].astype(np.uint64)
        hi = self.slots[:, 4:8].astype(np.uint64)
        return lo | (hi << np.uint64(32))

    def set_counters(self, c, rows=slice(None)):
        c = np.asarray(c, dtype=np.uint64)
        self.slots[rows, 0:4] = (c & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        self.slots[rows, 4:8] = (c >> np.uint64(32)).astype(np.uint32)

    def pending(self) -> np.ndarray:
        """bool [n]: the pending mark of every board."""
        pend = self.counters()[: n_waves(self.n), PEND]
        bits = (pend[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)
        return bits.reshape(-1)[: self.n].astype(bool)

    def load_into(self, eng):
        eng.load_state_dict(dict(self.state, blob=self.blob))


def slot_sums(c64: np.ndarray, n: int) -> tuple:
    """(episodes, illegal_ends, sum of G) over the slots the readers sum, as Python ints (mod 2^64 like the device)."""
    c = c64[: n_waves(n)]
    return tuple(int(c[:, k].sum(dtype=np.uint64)) for k in (EP, ILL, GAIN))


def books_return_sum(g_sum: int, scores: np.ndarray, pending: np.ndarray) -> int:
    """return_sum as the device defines it: G over all slots - the scores of the boards whose episode is running,
    mod 2^64, read as int64."""
    r = (g_sum - int(scores[~pending].astype(np.int64).sum())) % (1 << 64)
    return r - (1 << 64) if r >= 1 << 63 else r


def check_slots_match_stats(eng, blob: StateBlob = None) -> StateBlob:
    """The slots read from the blob add up to what ``episode_stats()`` reports, and the record region holds the
    engine's boards: the offsets above are the engine's.  Meaningful only once the counters are non-zero."""
    blob = StateBlob(eng) if blob is None else blob
    st = eng.episode_stats()
    ep, ill, g = slot_sums(blob.counters(), eng.n_envs)
    assert (st["episodes"], st["illegal_ends"]) == (ep, ill), "slot offset: episodes / illegal_ends"
    assert st["return_sum"] == books_return_sum(g, eng.get_scores(), blob.pending()), "slot offset: G / pending"
    assert np.array_equal(blob.records & 0x1F, eng.get_boards().reshape(-1, 16)), "record offset"
    return blob
