"""GPU: the second pass of a workgroup of the n-tuple reduced search kernel (g2048_ntuple_reduced_search), by
the means of tests/test_gpu_ntuple_adaptive_stride.py.  The kernel gives every board a workgroup, at most MAX_WORKGROUPS = 65 536
of them, and a workgroup keeps its table (NtupleDeepLds) for the next board of its stride loop -- here a board of ANOTHER DEPTH:
depth 0 writes V into the root sums that depth 1..4 add into, depth 1 never touches the entries that depth 2..4 fill, a leaf entry
of one board is a chance entry of the next, and a barrier that one depth takes and the other does not must still be taken by all
lanes or by none.

One batch of n = 65 536 + 7 boards under SCHEDULE.  H, with (empty cells, depth):
    0  CRAFTED[0]          1   4
    1  CRAFTED[2]          2   3
    2  WIDE_FANS[0]       15   2      one tile: the full table, 480 entries, half of them leaf entries
    3  empties_boards[4]   4   2
    4  TERMINAL            0   4      no legal move: an empty table
    5  empties_boards[6]   6   1
    6  empties_boards[8]   8   0
boards[0:7] = H, boards[7:65 536] = TERMINAL (dead: the workgroup passes its barriers and writes a dead board),
boards[65 536:] = H in reverse order -- workgroup j works on H[j] and then on H[6 - j]: real work on both passes.

Expected values: the host build's recursion of the definition (tests/host_ntuple_reduced), board by board at its own depth.  The
2 * 7 heavy rows bit for bit, the 65 529 fillers dead with depth SCHEDULE[0], compared on the device."""
import numpy as np
import pytest

from analysis_helpers import TERMINAL, g  # noqa: F401 (g: fixture)
from ntuple_adaptive_helpers import CRAFTED, ILLEGAL, SKIPPED, empties_boards, rows_at
from ntuple_deep_helpers import cached, dev, dev_u32, device_net, staged_net
from ntuple_helpers import TUPLES_8x4, random_net
from ntuple_reduced_helpers import REDUCE4, host_root, load_host_reduced
from ntuple_search_helpers import WIDE_FANS

pytestmark = pytest.mark.gpu
MAX_WORKGROUPS = (1 << 24) // 256      # kSearchMaxLanes / kBlock (g2048_kernels.hip): the grid cap of the workgroup-per-board kernels
SCHEDULE = (4, 4, 3, 3, 2, 2, 1, 1, 0, 0, 1, 2, 1, 0, 1, 2, 1)
DEPTHS = [4, 3, 2, 2, 4, 1, 0]


def heavy():
    e = empties_boards()
    return cached("reduced stride heavy", lambda: np.concatenate([CRAFTED[0:1], CRAFTED[2:3], WIDE_FANS[0:1], e[4:5], TERMINAL, e[6:7], e[8:9]]))


def batch():
    """uint8 [n, 16]: H, the fillers, H reversed."""
    def make():
        H = heavy()
        boards = np.repeat(TERMINAL, MAX_WORKGROUPS + len(H), 0)
        boards[:len(H)] = H
        boards[MAX_WORKGROUPS:] = H[::-1]
        return boards
    return cached("reduced stride batch", make)


def reference_net(name):
    return cached(("reduced stride net", name), lambda: random_net(TUPLES_8x4[:1], 41)) if name == "1x4" else staged_net()


def assert_inputs():
    H, boards = heavy(), batch()
    k, n = len(H), len(boards)
    assert k == 7 and n == MAX_WORKGROUPS + k and (boards[k:MAX_WORKGROUPS] == TERMINAL).all()
    depths = rows_at(SCHEDULE, H)[1].tolist()
    assert depths == DEPTHS and (H[2] == 0).sum() == 15
    second = rows_at(SCHEDULE, boards[MAX_WORKGROUPS:])[1].tolist()              # workgroup j: rows j, 65 536 + j
    pairs = list(zip(depths, second))
    assert pairs == list(zip(DEPTHS, DEPTHS[::-1]))
    for pair in ((4, 0), (0, 4), (3, 1), (1, 3), (2, 4), (4, 2)):
        assert pair in pairs, f"inputs: a depth-{pair[1]} board after a depth-{pair[0]} board"
    return k, n


def expected(name, R):
    """(action, value, depth) of H by the host build, once per (network, R)."""
    def make():
        H, lib, rnet = heavy(), load_host_reduced(), reference_net(name)
        act, val = np.zeros(len(H), np.uint8), np.zeros((len(H), 4), np.int64)
        for i, depth in enumerate(DEPTHS):
            a, v = host_root(lib, H[i:i + 1], depth, R, rnet)
            act[i], val[i] = a[0], v[0]
        return act, val, np.array(DEPTHS, np.uint8)
    want = cached(("reduced stride expected", name, R), make)
    legal = want[1] != ILLEGAL
    assert legal[[0, 1, 2, 3, 5, 6]].any(1).all() and not legal[4].any() and (np.abs(want[1][legal]) < 1 << 50).all()
    k = len(want[1])
    assert all((want[1][j] != want[1][k - 1 - j]).any() for j in range(k) if j != k - 1 - j), "inputs: the two boards of a pair differ in value"
    return want


def assert_batch(torch, got, want, k, on=None, where=""):
    """Rows 0..k-1 of ``got`` equal ``want`` and rows 65 536.. equal it reversed, where ``on`` (bool [n]) is set or None; the
    rows that are off are dead with depth SKIPPED and every filler is dead with depth SCHEDULE[0].  The fillers are compared on
    the device."""
    heavy_rows = np.concatenate([np.arange(k), np.arange(MAX_WORKGROUPS, MAX_WORKGROUPS + k)])
    want2 = tuple(np.concatenate([w, w[::-1]]) for w in want)
    if on is not None:
        off = ~on[heavy_rows]
        want2[0][off], want2[1][off], want2[2][off] = 0, ILLEGAL, SKIPPED
    idx = torch.as_tensor(heavy_rows, device="cuda:0")
    rows = tuple(None if t is None else t[idx].cpu().numpy() for t in got)
    for name, r, w in zip(("action", "value", "depth"), rows, want2):
        if r is not None:
            bad = np.nonzero((r.reshape(len(r), -1) != w.reshape(len(w), -1)).any(1))[0]
            assert len(bad) == 0, f"{where}: {name} differs on rows {heavy_rows[bad].tolist()}: first {r[bad[0]].tolist()} vs {w[bad[0]].tolist()}"
    if got[0] is not None:
        assert not bool(got[0][k:MAX_WORKGROUPS].any()), f"{where}: a filler's action"
    if got[1] is not None:
        assert bool((got[1][k:MAX_WORKGROUPS] == ILLEGAL).all()), f"{where}: a filler's values"
    if got[2] is not None:
        assert bool((got[2][k:MAX_WORKGROUPS] == SCHEDULE[0]).all()), f"{where}: a filler's depth"


@pytest.mark.parametrize("R", REDUCE4)
@pytest.mark.parametrize("name", ["1x4", "staged"])
def test_second_pass_on_plain_boards(g, torch_cuda, name, R):
    torch = torch_cuda
    k, n = assert_inputs()
    want = expected(name, R)
    net = device_net(g, reference_net(name))
    got = net.reduced_search(dev(torch, batch()), SCHEDULE, R)
    assert_batch(torch, got, want, k, where=f"{name}, R {R}")


@pytest.mark.parametrize("name, R", [("1x4", 2), ("staged", 1)])
def test_second_pass_on_an_engine_with_a_mask(g, torch_cuda, name, R):
    """The engine form, and the masked form twice: in the even pairs the first board is off and the second on, in the odd pairs
    the reverse -- o.active[i] at i >= 65 536, and a masked-out board before and after a depth-4 board; then the other way round."""
    torch = torch_cuda
    k, n = assert_inputs()
    want = expected(name, R)
    net = device_net(g, reference_net(name))
    eng = g.Batched2048(n, seed=3)
    try:
        eng.set_boards(batch())
        eng.set_scores(np.random.default_rng(1).integers(1, 1 << 24, n).astype(np.int32))     # the score-deficit bits are populated
        rec, clock = eng.records().clone(), eng.clock
        assert_batch(torch, eng.ntuple_reduced_search(net, SCHEDULE, R), want, k, where=f"{name}, engine")
        words = np.array([1, 7, 1 << 31, 0xffffffff], np.uint32)[np.arange(n) % 4]
        for flip in (0, 1):
            on = np.ones(n, bool)
            j = np.arange(k)
            on[j] = j % 2 != flip                           # the first board of pair j
            on[MAX_WORKGROUPS + j] = j % 2 == flip          # its second board
            mask = np.where(on, words, 0).astype(np.uint32)
            active = dev_u32(torch, mask)
            assert_batch(torch, eng.ntuple_reduced_search(net, SCHEDULE, R, active=active), want, k, on, f"{name}, masked, flip {flip}")
            assert np.array_equal(active.view(torch.int32).cpu().numpy().view(np.uint32), mask), "the mask is read only"
        assert torch.equal(eng.records(), rec) and eng.clock == clock
    finally:
        eng.close()


def test_second_pass_writes_only_the_fields_asked_for(g, torch_cuda):
    """out = (action, None, None) and out = (None, value, depth) on the n boards, 512 guard elements behind every buffer: the rows
    of the second pass are the last ones, and nothing past them is written."""
    torch = torch_cuda
    k, n = assert_inputs()
    want = expected("1x4", 1)
    net, d = device_net(g, reference_net("1x4")), dev(torch, batch())
    act = torch.full((n + 512,), 0x5A, dtype=torch.uint8, device="cuda")
    dep = torch.full((n + 512,), 0x5A, dtype=torch.uint8, device="cuda")
    val = torch.full((4 * n + 512,), 0x5A5A, dtype=torch.int64, device="cuda")
    res = net.reduced_search(d, SCHEDULE, 1, out=g.NTupleAdaptive(act[:n], None, None))
    assert res.value is None and res.depth is None
    assert_batch(torch, res, want, k, where="action only")
    assert bool((act[n:] == 0x5A).all()) and bool((val == 0x5A5A).all()) and bool((dep == 0x5A).all()), "action only: written past n, or elsewhere"
    act.fill_(0x5A)
    res = net.reduced_search(d, SCHEDULE, 1, out=g.NTupleAdaptive(None, val[:4 * n].view(n, 4), dep[:n]))
    assert res.action is None
    assert_batch(torch, res, want, k, where="value and depth")
    assert bool((val[4 * n:] == 0x5A5A).all()) and bool((dep[n:] == 0x5A).all()) and bool((act == 0x5A).all()), "value and depth: written past n, or actions written"
