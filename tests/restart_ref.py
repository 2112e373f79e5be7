"""Pure-Python reference of the midpoint restart (include/g2048.h "Midpoint restart") -- TEST INFRASTRUCTURE,
written from the definition in the header: one board after the other, Python integers, nothing shared with the product.  The
state is numpy arrays only so that a test can compare whole tensors; the rule itself runs on ints.  ``CASES`` are the engineered
states the host test and the GPU test both use, per rule and each one board: (name, pos, start, restarts, terminated)."""
from dataclasses import dataclass, field

import numpy as np

U32 = 0xffffffff


@dataclass(frozen=True)
class Rule:
    k: int = 4                # stride_log2
    C: int = 256              # capacity
    min_span: int = 64
    max_restarts: int = U32


@dataclass
class Events:
    """What happened in the steps of a State so far (the GPU test asserts that its run reaches each)."""
    restarts: int = 0
    refused_span: int = 0     # R < min_span
    refused_max: int = 0      # R >= min_span, restarts == max_restarts
    refused_progress: int = 0 # both hold, but q == 0 or S' <= S
    clamped: int = 0          # a restart with m >> k > C
    stores: int = 0
    log: list = field(default_factory=list)   # (step, board) of every restart


class State:
    """snap uint8 [C, n, 16], pos / start / restarts uint32 [n], zero-initialised."""

    def __init__(self, n, rule):
        self.n, self.rule = n, rule
        self.snap = np.zeros((rule.C, n, 16), np.uint8)
        self.pos = np.zeros(n, np.uint32)
        self.start = np.zeros(n, np.uint32)
        self.restarts = np.zeros(n, np.uint32)
        self.events = Events()
        self.steps = 0

    def step(self, records, terminated):
        """The restart step: ``records`` uint8 [n, 16] updated in place, ``terminated`` [n] (non-zero = true)."""
        r, ev = self.rule, self.events
        s = 1 << r.k
        for i in range(self.n):
            if not terminated[i]:
                if int(self.pos[i]) == U32:
                    continue
                p = int(self.pos[i]) + 1
                self.pos[i] = p
                q = p >> r.k
                if p & (s - 1) == 0 and 1 <= q <= r.C:
                    self.snap[q - 1, i] = records[i]
                    ev.stores += 1
                continue
            L, S = int(self.pos[i]), int(self.start[i])
            R = (L - S) & U32
            m = (S + (R >> 1)) & U32
            q = min(m >> r.k, r.C)
            S1 = q << r.k
            if R >= r.min_span and int(self.restarts[i]) < r.max_restarts and q >= 1 and S1 > S:
                records[i] = self.snap[q - 1, i]
                self.start[i] = self.pos[i] = S1
                self.restarts[i] = int(self.restarts[i]) + 1
                ev.restarts += 1
                ev.clamped += (m >> r.k) > r.C
                ev.log.append((self.steps, i))
            else:
                if R < r.min_span:
                    ev.refused_span += 1
                elif int(self.restarts[i]) >= r.max_restarts:
                    ev.refused_max += 1
                else:
                    ev.refused_progress += 1
                self.start[i] = self.pos[i] = self.restarts[i] = 0
        self.steps += 1


# ------------------------------------------------------------------------------------------------ the engineered states
# One rule for a whole batch (the rule is a launch argument): CASES[rule] = [(name, pos, start, restarts, terminated)].
BASE = Rule(k=2, C=4, min_span=8, max_restarts=3)        # s = 4: the snapshots of one lineage cover positions 4..16
CASES = {
    BASE: [
        ("p one before a stride multiple", 6, 0, 0, 0),            # p = 7: nothing stored
        ("p lands on a stride multiple", 7, 0, 0, 0),              # p = 8: slot 1
        ("p one after a stride multiple", 8, 0, 0, 0),             # p = 9
        ("p lands on slot C", 15, 4, 1, 0),                        # p = 16, q = 4 = C: the last slot
        ("p lands beyond slot C", 19, 0, 0, 0),                    # p = 20, q = 5 > C: not stored
        ("pos at the end of its range", U32, 0, 0, 0),             # stays, nothing stored
        ("pos one before the end", U32 - 1, 0, 0, 0),              # p = 2^32 - 1: counted, not a multiple of 4
        ("restart from the middle", 20, 0, 0, 1),                  # R = 20, m = 10, q = 2, S' = 8
        ("restart, q == C", 34, 0, 0, 1),                          # m = 17, m >> k = 4 = C: not a clamp
        ("restart, q == C + 1 clamped", 40, 0, 0, 1),              # m = 20, m >> k = 5 -> q = 4, S' = 16
        ("restart of a restarted run", 30, 8, 1, 1),               # R = 22, m = 19, q = 4, S' = 16 > 8
        ("restarted run moves on", 19, 8, 1, 1),                   # R = 11, m = 13, q = 3, S' = 12 > 8
        ("S' == S by the clamp", 60, 16, 2, 1),                    # m = 38 -> q = 4, S' = 16 == S: a fresh board
        ("R == min_span - 1", 7, 0, 0, 1),                         # refused
        ("R == min_span", 8, 0, 0, 1),                             # m = 4, q = 1, S' = 4: restarts
        ("R == min_span - 1 in a restarted run", 15, 8, 1, 1),
        ("restarts == max_restarts", 40, 0, 3, 1),                 # refused
        ("restarts == max_restarts - 1", 40, 0, 2, 1),             # the last one allowed
        ("fresh board ends at once", 0, 0, 0, 1),                  # R = 0
        ("pos at the end of its range, ended", U32, 0, 0, 1),      # m = 2^31 - 1 -> clamp to C, S' = 16
    ],
    Rule(k=0, C=4, min_span=2, max_restarts=2): [
        ("k = 0: every position is a snapshot", 0, 0, 0, 0),       # p = 1, q = 1
        ("k = 0: slot C", 3, 0, 0, 0),
        ("k = 0: beyond slot C", 4, 0, 0, 0),
        ("k = 0: restart at the exact middle", 6, 0, 0, 1),        # m = 3, S' = 3
        ("k = 0: R == min_span", 2, 0, 0, 1),                      # m = 1, S' = 1
        ("k = 0: R == 1", 1, 0, 0, 1),
        ("k = 0: restarted run, S' == S", 4, 3, 1, 1),             # R = 1 < 2
        ("k = 0: restarted run moves on", 4, 2, 1, 1),             # R = 2, m = 3 > 2
        ("k = 0: max reached", 4, 0, 2, 1),
    ],
    Rule(k=16, C=2, min_span=2, max_restarts=U32): [
        ("k = 16: p one before", 65534, 0, 0, 0),
        ("k = 16: p lands", 65535, 0, 0, 0),                       # p = 65536, q = 1
        ("k = 16: p one after", 65536, 0, 0, 0),
        ("k = 16: slot C", 2 * 65536 - 1, 0, 0, 0),
        ("k = 16: beyond slot C", 3 * 65536 - 1, 0, 0, 0),
        ("k = 16: q == 0, a fresh board", 100000, 0, 0, 1),        # m = 50000 < 65536
        ("k = 16: restart", 140000, 0, 0, 1),                      # m = 70000, q = 1
        ("k = 16: clamp", 400000, 0, 5, 1),                        # m = 200000, m >> 16 = 3 -> q = 2
        ("k = 16: max_restarts 2^32 - 1 reached", 400000, 0, U32, 1),
    ],
    Rule(k=3, C=4, min_span=2, max_restarts=9): [            # min_span < 2 s: the middle may lie in the stride the run began in
        ("S' == S: no progress, a fresh board", 14, 8, 1, 1),      # R = 6, m = 11, q = 1, S' = 8 == S
        ("S' > S by one stride", 24, 8, 1, 1),                     # R = 16, m = 16, q = 2, S' = 16
        ("q == 0: a fresh board", 6, 0, 0, 1),                     # R = 6, m = 3, q = 0
        ("q == 1", 16, 0, 0, 1),                                   # m = 8
    ],
    Rule(k=1, C=1, min_span=2, max_restarts=1): [
        ("C = 1: the one slot", 1, 0, 0, 0),                       # p = 2, q = 1
        ("C = 1: beyond it", 3, 0, 0, 0),
        ("C = 1: restart", 9, 0, 0, 1),                            # m = 4 -> q = 1 (clamped), S' = 2
        ("C = 1: restarted once already", 9, 2, 1, 1),             # max_restarts = 1
        ("C = 1: S' == S", 9, 2, 0, 1),                            # q = 1, S' = 2 == S
    ],
    Rule(k=4, C=8, min_span=1 << 31, max_restarts=7): [
        ("min_span 2^31: R one short", (1 << 31) - 1, 0, 0, 1),
        ("min_span 2^31: R == min_span", 1 << 31, 0, 0, 1),        # m = 2^30 -> clamp, S' = 128
        ("min_span 2^31: counted", 1 << 31, 0, 0, 0),
    ],
}


def case_state(rule, n):
    """A State of n boards and its records and terminated: board i is case i mod len(CASES[rule]).  Record i and every snapshot
    (slot j of board i) hold distinct bytes, so a record taken from another board or another slot does not go unnoticed."""
    cases = CASES[rule]
    st = State(n, rule)
    idx = np.arange(n) % len(cases)
    for name, arr in (("pos", 1), ("start", 2), ("restarts", 3)):
        getattr(st, name)[:] = np.array([c[arr] for c in cases], np.uint64)[idx].astype(np.uint32)
    terminated = np.array([c[4] for c in cases], np.uint8)[idx]
    rng = np.random.default_rng(1234 + rule.k)
    records = rng.integers(0, 256, (n, 16)).astype(np.uint8)
    st.snap[:] = rng.integers(0, 256, st.snap.shape).astype(np.uint8)
    return st, records, terminated


def expected_events(rule):
    """The events of one step of the cases of ``rule``, one board each."""
    st, records, terminated = case_state(rule, len(CASES[rule]))
    st.step(records, terminated)
    return st.events
