"""Pure-Python reference of the n-tuple expectimax (include/g2048.h "N-tuple expectimax") -- TEST
INFRASTRUCTURE ONLY.

Written from the definition on top of tests/ntuple_ref.py (``move``, ``value``, ``plain``) with Python integers and
Python's ``//`` (which floors), and nothing from the device header:

    A_0(a) = V(a)
    S_k(b) = max over legal d of ((g_d << F) + A_k(a_d));   0 when no move is legal
    A_k(a) = (sum over empty c of (9 * S_{k-1}(a, 2 in c) + S_{k-1}(a, 4 in c))) // (10 * E(a))   for k >= 1
    value[d] = (g_d << F) + A_D(a_d), ILLEGAL where d is illegal; action = the smallest d of largest value, 0 when none

A cell is empty when its exponent equals 0.  ``Trace`` counts what a search met, so that a test can show from the
reference alone that its input reaches the edge it names.
"""
from __future__ import annotations

import numpy as np

import ntuple_ref as ref

ILLEGAL = ref.ILLEGAL


class Trace:
    """chance: chance nodes; negative_inexact: those whose sum was negative and not divisible by 10E; terminal_children:
    children of a chance node with no legal move (S = 0); root_ties: boards whose largest root value two moves share;
    root_items: {number of chance items 2E of a root direction's afterstate: how many legal root directions had it}."""

    def __init__(self):
        self.chance = self.negative_inexact = self.terminal_children = self.root_ties = 0
        self.root_items = {}

    def __repr__(self):
        return (f"Trace(chance={self.chance}, negative_inexact={self.negative_inexact}, "
                f"terminal_children={self.terminal_children}, root_ties={self.root_ties})")


def after_value(a, k, net, trace=None):
    """A_k(a)."""
    if k == 0:
        return ref.value(a, net)
    empty = [c for c in range(16) if a[c] == 0]
    total = 0
    for c in empty:
        for exponent, weight in ((1, 9), (2, 1)):
            child = a[:c] + (exponent,) + a[c + 1:]
            total += weight * state_value(child, k - 1, net, trace, child_of_chance=True)
    if trace is not None:
        trace.chance += 1
        trace.negative_inexact += total < 0 and total % (10 * len(empty)) != 0
    return total // (10 * len(empty))


def state_value(b, k, net, trace=None, child_of_chance=False):
    """S_k(b)."""
    best = None
    for d in range(4):
        a, g, legal = ref.move(b, d)
        if legal:
            q = (g << net.frac_bits) + after_value(a, k, net, trace)
            best = q if best is None or q > best else best
    if best is None:
        if trace is not None and child_of_chance:
            trace.terminal_children += 1
        return 0
    return best


def search(board, depth, net, trace=None):
    """(value[4], action) of one board."""
    b = ref.plain(board)
    value = [ILLEGAL] * 4
    for d in range(4):
        a, g, legal = ref.move(b, d)
        if legal:
            value[d] = (g << net.frac_bits) + after_value(a, depth, net, trace)
            if trace is not None:
                items = 2 * sum(1 for x in a if x == 0)
                trace.root_items[items] = trace.root_items.get(items, 0) + 1
    legal = [d for d in range(4) if value[d] != ILLEGAL]
    if not legal:
        return value, 0
    action = max(legal, key=lambda d: (value[d], -d))
    if trace is not None:
        trace.root_ties += sum(value[d] == value[action] for d in legal) > 1
    return value, action


def search_batch(boards, depth, net, trace=None):
    """(action uint8 [n], value int64 [n, 4])."""
    boards = np.asarray(boards).reshape(-1, 16)
    act, val = np.zeros(len(boards), np.uint8), np.zeros((len(boards), 4), np.int64)
    for i, b in enumerate(boards):
        val[i], act[i] = search(b, depth, net, trace)
    return act, val
