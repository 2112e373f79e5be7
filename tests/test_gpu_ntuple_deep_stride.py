"""GPU: the second pass of a workgroup of the n-tuple deep search kernel (g2048_ntuple_deep_search) with a
full table.  The kernel gives every board a workgroup, at most MAX_WORKGROUPS = 65 536 of them, and a workgroup keeps its table
of level-1 items in LDS (NtupleDeepLds) for the next board of its stride loop: the closing barrier, the reset of the root sums
and of the entries' chance sums, and whatever the last board left above the new board's item count matter on that pass only.

One batch of n = 65 536 + 19 boards.  H = WIDE_FANS (10 boards), the six boards of near_full(2), PAIR_ONLY, ONE_LEGAL, TERMINAL;
boards[0:19] = H, boards[19:65 536] = TERMINAL (no legal move: no items, the workgroup passes its barriers and writes a dead
board), boards[65 536:] = H in reverse order -- workgroup j works on H[j] and then on H[18 - j].  Level-1 items of H, from
ntuple_deep_helpers.children_of alone (120 = the full table, 480 entries):
    120, 60, 88, 112, 96, 96, 36, 16, 28, 72, 8, 6, 20, 16, 16, 16, 4, 8, 0
so the pairs (first pass, second pass) are (120, 0), (60, 8), (88, 4), (112, 16), (96, 16), (96, 16), (36, 20), (16, 6), (28, 8),
(72, 72) and their reverses: a smaller table after a larger one, a larger after a smaller, an empty one after the full one
and the full one after an empty one.  The tests assert all four.

Expected values from the definition: compose_depth3(H) over search(.., 2) at depth 3, search(H, 2) itself at depth 2; the 2 * 19
heavy rows bit for bit, the 65 517 fillers dead (compared on the device).  Networks: one 4-tuple (uniform, T = 1) and the
three-stage network of two 4-tuples of ntuple_deep_helpers.staged_net().

Device time of one launch of the batch on the MI355X, measured with the tests' own inputs (events around the call, four
launches each; the plain, the engine and the masked form with every board on take the same time):
    one 4-tuple   depth 2: 0.22 ms    depth 3: 15.8 ms
    staged, T = 2 depth 2: 0.32 ms    depth 3: 27.1 ms
A test makes one to four such launches and the depth-2 calls of its expected values; the whole module takes 5 s.

Tried once on scratch builds of the library (never committed), against this module:
    without ``l.root_sum[lane] = 0`` (ntuple_deep_root)    all 10 tests fail
    without ``l.acc[e] = 0`` (ntuple_deep_expand)          all 10 tests fail
    without the MASKED kernel's read of o.active           the 4 masked tests fail
    without the closing __syncthreads() of the stride loop all 10 tests pass.  Between the last barrier of a board and the first
        one of the next, only lanes 0..3 write the table (root) and only lane 0 reads it (finish): all of them lie in wavefront 0,
        which runs its instructions in order, and the other wavefronts wait at the barrier behind root.  The hardware therefore
        never shows that race with this split of the steps; the barrier guards a change of who runs root or finish.
"""
import numpy as np
import pytest

from analysis_helpers import ONE_LEGAL, TERMINAL, g  # noqa: F401 (g: fixture)
from ntuple_deep_helpers import ILLEGAL, cached, children_of, compose_depth3, dev, dev_u32, device_net, near_full, staged_net, to_np
from ntuple_helpers import TUPLES_8x4, random_net
from ntuple_search_helpers import PAIR_ONLY, WIDE_FANS

pytestmark = pytest.mark.gpu
MAX_WORKGROUPS = (1 << 24) // 256      # kSearchMaxLanes / kBlock (g2048_kernels.hip): the grid cap of the deep search kernel
ITEMS = [120, 60, 88, 112, 96, 96, 36, 16, 28, 72, 8, 6, 20, 16, 16, 16, 4, 8, 0]
CASES = [(name, depth) for name in ("1x4", "staged") for depth in (2, 3)]


def heavy():
    return cached("stride heavy", lambda: np.concatenate([WIDE_FANS, near_full(2)[0], PAIR_ONLY, ONE_LEGAL, TERMINAL]))


def batch():
    """uint8 [n, 16]: H, the fillers, H reversed."""
    def make():
        H = heavy()
        boards = np.repeat(TERMINAL, MAX_WORKGROUPS + len(H), 0)
        boards[:len(H)] = H
        boards[MAX_WORKGROUPS:] = H[::-1]
        return boards
    return cached("stride batch", make)


def reference_net(name):
    return cached(("stride net", name), lambda: random_net(TUPLES_8x4[:1], 41)) if name == "1x4" else staged_net()


def assert_inputs():
    """From children_of alone: the item counts of H, and what the pairs of one workgroup's two passes cover."""
    H, boards = heavy(), batch()
    k, n = len(H), len(boards)
    assert k == 19 and n == MAX_WORKGROUPS + k and (boards[k:MAX_WORKGROUPS] == TERMINAL).all()

    def count(b):
        return [sum(len(lst) for lst in per if lst is not None) for per in children_of(b)[0]]
    items = cached("stride items", lambda: count(H))
    assert items == ITEMS and count(TERMINAL) == [0]
    pairs = [(items[j], count(boards[MAX_WORKGROUPS + j:MAX_WORKGROUPS + j + 1])[0]) for j in range(k)]   # workgroup j: rows j, 65 536 + j
    assert pairs == list(zip(ITEMS, ITEMS[::-1]))
    assert any(0 < b < a for a, b in pairs) and any(0 < a < b for a, b in pairs), "inputs: a smaller table after a larger one and the reverse"
    assert (120, 0) in pairs and (0, 120) in pairs, "inputs: an empty table after the full one and the reverse"
    return k, n


def expected(g, torch, name, depth):
    """(action, value) of H from the definition, once per (network, depth)."""
    def make():
        rnet = reference_net(name)
        net = device_net(g, rnet)
        if depth == 2:
            return to_np(net.search(dev(torch, heavy()), 2))
        want, widest, dead = compose_depth3(heavy(), rnet.frac_bits, lambda kids: net.search(dev(torch, kids), 2).value.cpu().numpy())
        assert widest == 30 and dead >= 1
        return want
    want = cached(("stride expected", name, depth), make)
    legal = want[1] != ILLEGAL
    assert legal[0].all() and not legal[18].any() and (np.abs(want[1][legal]) < 1 << 50).all()
    k = len(want[1])
    assert all((want[1][j] != want[1][k - 1 - j]).any() for j in range(k) if j != k - 1 - j), "inputs: the two boards of a pair differ in value"
    return want


def assert_batch(torch, got, want, k, on=None, where=""):
    """Rows 0..k-1 of ``got`` equal ``want`` and rows 65 536.. equal it reversed, where ``on`` (bool [n]) is set or None; the
    rows that are off and every filler are dead.  The fillers are compared on the device."""
    heavy_rows = np.concatenate([np.arange(k), np.arange(MAX_WORKGROUPS, MAX_WORKGROUPS + k)])
    want2 = tuple(np.concatenate([w, w[::-1]]) for w in want)
    if on is not None:
        off = ~on[heavy_rows]
        want2[0][off], want2[1][off] = 0, ILLEGAL
    idx = torch.as_tensor(heavy_rows, device="cuda:0")
    rows = tuple(None if t is None else t[idx].cpu().numpy() for t in got)
    for name, r, w in zip(("action", "value"), rows, want2):
        if r is not None:
            bad = np.nonzero((r.reshape(len(r), -1) != w.reshape(len(w), -1)).any(1))[0]
            assert len(bad) == 0, f"{where}: {name} differs on rows {heavy_rows[bad].tolist()}: first {r[bad[0]].tolist()} vs {w[bad[0]].tolist()}"
    if got[0] is not None:
        assert not bool(got[0][k:MAX_WORKGROUPS].any()), f"{where}: a filler's action"
    if got[1] is not None:
        assert bool((got[1][k:MAX_WORKGROUPS] == ILLEGAL).all()), f"{where}: a filler's values"


# ------------------------------------------------------------------------------------------------ plain boards
@pytest.mark.parametrize("name, depth", CASES)
def test_second_pass_on_plain_boards(g, torch_cuda, name, depth):
    torch = torch_cuda
    k, n = assert_inputs()
    want = expected(g, torch, name, depth)
    net = device_net(g, reference_net(name))
    got = net.deep_search(dev(torch, batch()), depth)
    assert_batch(torch, got, want, k, where=f"{name} depth {depth}")


# ------------------------------------------------------------------------------------------------ the engine, the mask
@pytest.mark.parametrize("name, depth", CASES)
def test_second_pass_on_an_engine_with_a_mask(g, torch_cuda, name, depth):
    """The engine form, and the masked form twice: in the even pairs the first board is off and the second on, in the odd pairs
    the reverse -- o.active[i] at i >= 65 536, and a masked-out board before and after a full table; then the other way round."""
    torch = torch_cuda
    k, n = assert_inputs()
    want = expected(g, torch, name, depth)
    net = device_net(g, reference_net(name))
    eng = g.Batched2048(n, seed=3)
    try:
        eng.set_boards(batch())
        eng.set_scores(np.random.default_rng(1).integers(1, 1 << 24, n).astype(np.int32))     # the score-deficit bits are populated
        rec, clock = eng.records().clone(), eng.clock
        assert_batch(torch, eng.ntuple_deep_search(net, depth), want, k, where=f"{name} depth {depth}, engine")
        words = np.array([1, 7, 1 << 31, 0xffffffff], np.uint32)[np.arange(n) % 4]
        for flip in (0, 1):
            on = np.ones(n, bool)
            j = np.arange(k)
            on[j] = j % 2 != flip                           # the first board of pair j
            on[MAX_WORKGROUPS + j] = j % 2 == flip          # its second board
            assert on[0] == bool(flip) and on[MAX_WORKGROUPS + k - 1] != bool(flip), "inputs: the 120-item board off on a first pass, on on a second"
            mask = np.where(on, words, 0).astype(np.uint32)
            active = dev_u32(torch, mask)
            assert_batch(torch, eng.ntuple_deep_search(net, depth, active=active), want, k, on, f"{name} depth {depth}, masked, flip {flip}")
            assert np.array_equal(active.view(torch.int32).cpu().numpy().view(np.uint32), mask), "the mask is read only"
        assert torch.equal(eng.records(), rec) and eng.clock == clock
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ partial outputs
@pytest.mark.parametrize("name", ["1x4", "staged"])
def test_second_pass_writes_only_the_fields_asked_for(g, torch_cuda, name):
    """out = (action, None) and out = (None, value) on the n boards at depth 3, 512 guard elements behind either buffer: the rows
    of the second pass are the last ones, and nothing past them is written."""
    torch = torch_cuda
    k, n = assert_inputs()
    want = expected(g, torch, name, 3)
    net, d = device_net(g, reference_net(name)), dev(torch, batch())
    act = torch.full((n + 512,), 0x5A, dtype=torch.uint8, device="cuda")
    val = torch.full((4 * n + 512,), 0x5A5A, dtype=torch.int64, device="cuda")
    res = net.deep_search(d, 3, out=g.NTupleSearch(act[:n], None))
    assert res.value is None
    assert_batch(torch, res, want, k, where=f"{name}, action only")
    assert bool((act[n:] == 0x5A).all()) and bool((val == 0x5A5A).all()), "action only: written past n, or values written"
    act.fill_(0x5A)
    res = net.deep_search(d, 3, out=g.NTupleSearch(None, val[:4 * n].view(n, 4)))
    assert res.action is None
    assert_batch(torch, res, want, k, where=f"{name}, value only")
    assert bool((val[4 * n:] == 0x5A5A).all()) and bool((act == 0x5A).all()), "value only: written past n, or actions written"
