"""Pure-Python reference of the n-tuple reduced search (include/g2048.h "N-tuple reduced search") -- TEST
INFRASTRUCTURE ONLY.

Written from the definition on top of tests/ntuple_ref.py (``move``, ``value``, ``plain``) with Python integers and
Python's ``//`` (which floors), and nothing from the device header.  R = reduce4 in 1..2:

    A^R_0(a) = V(a)
    S^R_k(b) = max over legal d of ((g_d << F) + A^R_k(a_d));   0 when no move is legal
    A^R_k(a) = (sum over empty c of (9 * S^R_{k-1}(a, 2 in c) + S^R_{max(k-1-R, 0)}(a, 4 in c))) // (10 * E(a))   for k >= 1
    value[d] = (g_d << F) + A^R_D(a_d), ILLEGAL where d is illegal; action = the smallest d of largest value, 0 when none

A cell is empty when its exponent equals 0.  ``Trace`` counts what a search met, so that a test can show from the reference
alone that its input reaches the states it names; ``evaluations`` counts the leaves, V look-ups, which is what the search costs.
"""
from __future__ import annotations

import numpy as np

import ntuple_ref as ref

ILLEGAL = ref.ILLEGAL


class Trace:
    """chance: chance nodes; negative_inexact: those whose sum was negative and not divisible by 10E; terminal_children: children
    of a chance node with no legal move (S = 0); terminal_level1: those among the children of a root afterstate; root_ties:
    boards whose largest root value two moves share; leaf_beside_units: cells of a root afterstate whose 4 child is searched at
    depth 0 and has a legal move while its 2 sibling has a legal move and is searched at depth >= 1 (a leaf entry next to
    entries with work units); level1_depths: {remaining depth r1 of a level-1 child: how many}; evaluations: V look-ups."""

    def __init__(self):
        self.chance = self.negative_inexact = self.terminal_children = self.terminal_level1 = self.root_ties = 0
        self.leaf_beside_units = self.evaluations = 0
        self.level1_depths = {}


def has_move(b):
    return any(ref.move(b, d)[2] for d in range(4))


def after_value(a, k, R, net, trace=None, level=1):
    """A^R_k(a); ``level`` 1 is the afterstate of a root move."""
    if k == 0:
        if trace is not None:
            trace.evaluations += 1
        return ref.value(a, net)
    empty = [c for c in range(16) if a[c] == 0]
    total = 0
    for c in empty:
        kids = []
        for exponent, weight, below in ((1, 9, k - 1), (2, 1, max(k - 1 - R, 0))):
            child = a[:c] + (exponent,) + a[c + 1:]
            kids.append((child, below))
            if trace is not None and level == 1:
                trace.level1_depths[below] = trace.level1_depths.get(below, 0) + 1
            total += weight * state_value(child, below, R, net, trace, level)
        if trace is not None and level == 1:
            (two, k2), (four, k4) = kids
            trace.leaf_beside_units += k4 == 0 and k2 >= 1 and has_move(four) and has_move(two)
    if trace is not None:
        trace.chance += 1
        trace.negative_inexact += total < 0 and total % (10 * len(empty)) != 0
    return total // (10 * len(empty))


def state_value(b, k, R, net, trace=None, level=0):
    """S^R_k(b), b a child of a chance node of ``level``."""
    best = None
    for d in range(4):
        a, g, legal = ref.move(b, d)
        if legal:
            q = (g << net.frac_bits) + after_value(a, k, R, net, trace, level + 1)
            best = q if best is None or q > best else best
    if best is None:
        if trace is not None:
            trace.terminal_children += 1
            trace.terminal_level1 += level == 1
        return 0
    return best


def search(board, depth, R, net, trace=None):
    """(value[4], action) of one board."""
    assert 0 <= depth <= 4 and 1 <= R <= 2
    b = ref.plain(board)
    value = [ILLEGAL] * 4
    for d in range(4):
        a, g, legal = ref.move(b, d)
        if legal:
            value[d] = (g << net.frac_bits) + after_value(a, depth, R, net, trace)
    legal = [d for d in range(4) if value[d] != ILLEGAL]
    if not legal:
        return value, 0
    action = max(legal, key=lambda d: (value[d], -d))
    if trace is not None:
        trace.root_ties += sum(value[d] == value[action] for d in legal) > 1
    return value, action


def search_batch(boards, depth, R, net, trace=None):
    """(action uint8 [n], value int64 [n, 4])."""
    boards = np.asarray(boards).reshape(-1, 16)
    act, val = np.zeros(len(boards), np.uint8), np.zeros((len(boards), 4), np.int64)
    for i, b in enumerate(boards):
        val[i], act[i] = search(b, depth, R, net, trace)
    return act, val
