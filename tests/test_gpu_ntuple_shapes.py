"""GPU: every instantiation of the n-tuple kernels -- tuple counts T = 1..8, lengths L = 1..6, search depths 1 and 2, the
plain and the engine form -- the depth-2 item walk on wide chance fans, values at the bounds the header states, and
batches that leave a wave partly filled, against the pure-Python references tests/ntuple_ref.py, ntuple_search_ref.py and
ntuple_tc_ref.py, bit for bit.  Every test shows from the reference (never from the code under test) that its input
reaches the edge it names.

Network T of the tuple-count tests is the first T lists of TUPLES_8x4 with the first T tables of one weight array, so the
reference's outputs for T - 1 are those of a launch that took the neighbouring instantiation: they must differ.

CPU time of the reference work, measured on one core with the tests' own inputs (the device work is milliseconds):
  evaluate / values / search depth 1, T = 1..8:  0.9 .. 2.8 s each      search depth 2, T = 1..8:   1.1 .. 3.3 s each
  update and tc_update, T = 1..8:  below 0.2 s each                     lengths L = 1..6:           1.0 .. 2.0 s each
  T = 8, L = 6 corner:  6.5 s, and 1.4 s once for its tables            its tc_update:              below 0.1 s
  wide fans, T = 1 / 2:  11 s / 16 s                                    bounds, six cases:          5 .. 6 s each
  ragged n, five cases:  below 0.1 s each (T = 3 of the cases above, cached; 2.6 s when run alone)
"""
import numpy as np
import pytest

import ntuple_ref as ref
import ntuple_search_ref as sref
import ntuple_tc_ref as tcref
from analysis_helpers import ONE_LEGAL, TERMINAL, assert_rows_periodic, g, mid_game, mixed_boards, random_boards  # noqa: F401 (g: fixture)
from ntuple_deep_helpers import bound_fill
from ntuple_helpers import EVAL_NAMES, TUPLES_3xL, TUPLES_8x4, TUPLES_8x6, assert_eval_equal, random_net
from ntuple_search_helpers import PAIR_ONLY, SEARCH_NAMES, WIDE_FANS, assert_search_equal
from ntuple_tc_helpers import EDGE_PAIRS, assert_tables_equal, edge_deltas, preload

pytestmark = pytest.mark.gpu

INT32_MAX, INT32_MIN = (1 << 31) - 1, -(1 << 31)
TIE = np.array([[0] * 5 + [3] + [0] * 10], np.uint8)    # the four afterstates are images of one another: four equal values
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def boards_64():
    """60 mixed boards, the tie board, PAIR_ONLY, ONE_LEGAL and TERMINAL: one board more than four waves of evaluate."""
    return cached("boards", lambda: np.concatenate([mixed_boards(60, 81), TIE, PAIR_ONLY, ONE_LEGAL, TERMINAL]))


def near_full_12():
    return cached("near full", lambda: np.concatenate([mid_game(10, 82, max_empty=2), PAIR_ONLY, TERMINAL]))


def net_of(T):
    """Network T: the first T lists of TUPLES_8x4 and the first T tables of one array of full-range int32 weights."""
    w = cached("weights", lambda: np.random.default_rng(83).integers(INT32_MIN, INT32_MAX + 1, size=(8, 16 ** 4)))
    return ref.Net(TUPLES_8x4[:T], 10, w[:T])


def device_net(g, rnet):
    """An NTupleNet on the GPU with the shape and weights of a reference network."""
    import torch
    net = g.NTupleNet(rnet.tuples, frac_bits=rnet.frac_bits, device="cuda:0")
    net.weights.copy_(torch.as_tensor(rnet.weights.astype(np.int32)))
    return net


def device_tc(g, torch, net, rtc):
    tc = g.NTupleTC(net)
    tc.err.copy_(torch.as_tensor(rtc.err))
    tc.mag.copy_(torch.as_tensor(rtc.mag_i64()))
    return tc


def dev(torch, a):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda:0")


def to_np(e):
    return tuple(None if t is None else t.cpu().numpy() for t in e)


def search_ref(boards, depth, rnet):
    """((action, value), trace) of the reference."""
    trace = sref.Trace()
    return sref.search_batch(boards, depth, rnet, trace), trace


def check_both_forms(g, torch, boards, rnet, evaluate=None, values=None, searches=()):
    """The plain and the engine form of evaluate, values (plain only) and search at every (depth, want) of ``searches``
    equal the reference's outputs; the engine form leaves the engine as it was."""
    net, d = device_net(g, rnet), dev(torch, boards)
    if evaluate is not None:
        assert_eval_equal(to_np(net.evaluate(d)), evaluate, boards, "evaluate, plain")
    if values is not None:
        assert np.array_equal(net.values(d).cpu().numpy(), values), "values"
    for depth, want in searches:
        assert_search_equal(to_np(net.search(d, depth)), want, boards, f"search depth {depth}, plain")
    eng = g.Batched2048(len(boards), seed=3)
    try:
        eng.set_boards(boards % 32)
        eng.set_scores(np.random.default_rng(1).integers(1, 1 << 24, len(boards)).astype(np.int32))   # deficit bits populated
        rec = eng.records().clone()
        if evaluate is not None:
            assert_eval_equal(to_np(eng.ntuple_evaluate(net)), evaluate, boards, "evaluate, engine")
        for depth, want in searches:
            assert_search_equal(to_np(eng.ntuple_search(net, depth)), want, boards, f"search depth {depth}, engine")
        assert torch.equal(eng.records(), rec)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------ 1. every tuple count and length
def shallow(T):
    """The reference on boards_64 under network T: (evaluate, values, (search depth 1, trace))."""
    return cached(("shallow", T), lambda: (ref.evaluate_batch(boards_64(), net_of(T)), ref.values_batch(boards_64(), net_of(T)),
                                           search_ref(boards_64(), 1, net_of(T))))


def deep(T):
    return cached(("deep", T), lambda: search_ref(near_full_12(), 2, net_of(T)))


@pytest.mark.parametrize("T", range(1, 9))
def test_every_tuple_count_evaluate_values_search_depth_1(g, torch_cuda, T):
    boards = boards_64()
    want_e, want_v, (want_s, trace) = shallow(T)
    q = want_e[0]
    assert len(set(q[60].tolist())) == 1 and q[60, 0] != ref.ILLEGAL and want_e[1][60] == 0          # the tie: smallest direction
    assert (q[62] != ref.ILLEGAL).sum() == 1 and (q[63] == ref.ILLEGAL).all() and (want_s[1][63] == sref.ILLEGAL).all()
    assert trace.negative_inexact > 0 and trace.terminal_children >= 2 and len(set(want_s[0].tolist())) == 4
    if T > 1:   # the neighbouring instantiation on the same weights computes something else
        prev_e, prev_v, (prev_s, _) = shallow(T - 1)
        assert (prev_e[0] != q).any() and (prev_e[4] != want_e[4]).any() and (prev_v != want_v).any() and (prev_s[1] != want_s[1]).any()
    check_both_forms(g, torch_cuda, boards, net_of(T), want_e, want_v, [(1, want_s)])


@pytest.mark.parametrize("T", range(1, 9))
def test_every_tuple_count_search_depth_2(g, torch_cuda, T):
    boards = near_full_12()
    want, trace = deep(T)
    assert ((boards == 0).sum(1) <= 2).all() and trace.negative_inexact > 0 and trace.terminal_children >= 2
    assert (want[1][-1] == sref.ILLEGAL).all() and (want[1][:-1] != sref.ILLEGAL).any(1).all()
    if T > 1:
        assert (deep(T - 1)[0][1] != want[1]).any()
    check_both_forms(g, torch_cuda, boards, net_of(T), searches=[(2, want)])


@pytest.mark.parametrize("T", range(1, 9))
def test_every_tuple_count_update(g, torch_cuda, T):
    torch = torch_cuda
    boards, rnet = boards_64(), net_of(T)
    deltas = np.random.default_rng(84).integers(-(1 << 30), 1 << 30, len(boards))
    deltas[::9] = 0
    deltas[[1, 2, 3, 4]] = [1 << 45, -(1 << 45), 5, -5]
    assert [ref.step_of(x, 3) for x in deltas[:5]] == [0, INT32_MAX, INT32_MIN, 0, -1]   # both saturations, a floor to 0 and to -1
    after, trace = rnet.copy(), {}
    ref.update(after, boards, deltas, 3, trace)
    assert trace["zero"] >= 9 and trace["sat"] == 2 and (deltas > 0).any() and (deltas < 0).any()
    assert (after.weights[T - 1] != rnet.weights[T - 1]).any()     # the last table is written: the (T - 1)-network leaves it alone
    net = device_net(g, rnet)
    net.update(dev(torch, boards), dev(torch, deltas), 3)
    assert_tables_equal([net.weights.cpu().numpy().astype(np.int64)], [after.weights], ["weights"])


@pytest.mark.parametrize("T", range(1, 9))
def test_every_tuple_count_tc_update(g, torch_cuda, T):
    torch = torch_cuda
    boards, rnet = boards_64(), net_of(T)
    rtc = preload(rnet, 85, boards[:8])
    deltas = edge_deltas(len(boards), 86)
    after, after_tc, trace = rnet.copy(), rtc.copy(), {}
    tcref.tc_update(after, after_tc, boards, deltas, 0, 3, trace)
    assert trace["zero"] >= 7 and trace["clamp_d"] >= 4 and trace["multi"] > 0 and trace["k"] > 0 and trace["rate0"] > 0
    assert trace["rate1"] > 0 and trace["clamp_m"] > 0 and trace["sat"] > 0
    for new, old in ((after.weights, rnet.weights), (after_tc.err, rtc.err), (after_tc.mag, rtc.mag)):
        assert (new[T - 1] != old[T - 1]).any()         # the last tables are written: the (T - 1)-network leaves them alone
    net = device_net(g, rnet)
    tc = device_tc(g, torch, net, rtc)
    net.tc_update(dev(torch, boards), dev(torch, deltas), 0, tc, 3)
    assert_tables_equal((net.weights.cpu().numpy().astype(np.int64), tc.err.cpu().numpy(), tc.mag.cpu().numpy()),
                        (after.weights, after_tc.err, after_tc.mag_i64()))


@pytest.fixture(scope="module")
def net_8x6():
    """The reference network of the corner T = 8, L = 6 (1 GiB of int64 on the host), once and freed with the module."""
    return random_net(TUPLES_8x6, 87)


@pytest.mark.parametrize("L", range(1, 7))
def test_every_length_evaluate_and_search_depth_1(g, torch_cuda, net_8x6, L):
    """T = 3 with the first L cells of three 6-cell lists; L = 6 reads the first three tables of the corner's network."""
    boards = boards_64()
    if L < 6:
        rnet = random_net(TUPLES_3xL[L], 88 + L)
    else:
        rnet = ref.Net.__new__(ref.Net)
        rnet.tuples, rnet.frac_bits, rnet.weights = list(TUPLES_3xL[6]), 10, net_8x6.weights[:3]
    hits = [h for b in boards for h in tcref.hits_of(b, rnet)]
    assert {t for t, _ in hits} == {0, 1, 2} and max(i for _, i in hits) >= 15 << (4 * (L - 1))   # the top nibble is used
    want_e, (want_s, trace) = ref.evaluate_batch(boards, rnet), search_ref(boards, 1, rnet)
    assert trace.negative_inexact > 0 and len(set(want_s[0].tolist())) == 4
    check_both_forms(g, torch_cuda, boards, rnet, want_e, ref.values_batch(boards, rnet), [(1, want_s)])


def test_corner_8_tuples_of_6_cells(g, torch_cuda, net_8x6):
    """T = 8, L = 6: evaluate and depth 1 on boards_64, depth 2 on four near-full boards; the last entry of the last table
    is read."""
    boards = np.concatenate([boards_64(), np.array([[15, 16, 17, 31] * 4], np.uint8)])
    assert (7, 16 ** 6 - 1) in tcref.hits_of(boards[-1], net_8x6)
    want_e, (want_s, trace) = ref.evaluate_batch(boards, net_8x6), search_ref(boards, 1, net_8x6)
    assert trace.negative_inexact > 0 and len(set(want_s[0].tolist())) == 4
    check_both_forms(g, torch_cuda, boards, net_8x6, want_e, ref.values_batch(boards, net_8x6), [(1, want_s)])
    near = near_full_12()[[0, 1, 2, 10]]
    want_2, trace = search_ref(near, 2, net_8x6)
    assert trace.chance > 100 and trace.terminal_children >= 2
    check_both_forms(g, torch_cuda, near, net_8x6, searches=[(2, want_2)])


def test_corner_8_tuples_of_6_cells_tc_update(g, torch_cuda):
    """T = 8, L = 6 for TC: 2 GiB of accumulators on the GPU only; the reference keeps the entries it wrote."""
    torch = torch_cuda
    rnet, rtc = tcref.sparse_net(TUPLES_8x6)
    boards = np.concatenate([random_boards(40, 89), np.array([[15, 16, 17, 31] * 4], np.uint8)])
    hits = [h for b in boards for h in tcref.hits_of(b, rnet)]
    assert (7, 16 ** 6 - 1) in hits and {t for t, _ in hits} == set(range(8))
    net = g.NTupleNet(TUPLES_8x6, device="cuda:0")
    tc = g.NTupleTC(net)
    for k, (t, i) in enumerate(hits[:128]):             # a few accumulators at the edges of the rate
        e, a = EDGE_PAIRS[k % len(EDGE_PAIRS)]
        rtc.err[t, i], rtc.mag[t, i] = e, a
        tc.err[t, i], tc.mag[t, i] = e, a - (1 << 64) if a >= 1 << 63 else a
    trace = {}
    for seed, shift in ((90, 0), (91, 3)):              # the second call learns at the rates the first one left
        deltas = edge_deltas(len(boards), seed)
        tcref.tc_update(rnet, rtc, boards, deltas, shift, 3, trace)
        net.tc_update(dev(torch, boards), dev(torch, deltas), shift, tc, 3)
    assert trace["k"] > 0 and trace["rate1"] > 0 and trace["rate0"] > 0 and trace["clamp_d"] > 0
    for name, got, want in (("weights", net.weights, rnet.weights), ("err", tc.err, rtc.err), ("mag", tc.mag, rtc.mag)):
        keys = sorted(want)
        rows, cols = (torch.as_tensor([k[x] for k in keys], device="cuda") for x in (0, 1))
        vals = np.array([want[k] - (1 << 64) if want[k] >= 1 << 63 else want[k] for k in keys], np.int64)   # mag: the int64 pattern
        assert np.array_equal(got[rows, cols].cpu().numpy().astype(np.int64), vals), name
        assert int(torch.count_nonzero(got)) == int(np.count_nonzero(vals)), name     # nothing else was written


# ------------------------------------------------------------------------------------ 2. wide chance fans at depth 2
@pytest.mark.parametrize("T", [1, 2])
def test_wide_chance_fans(g, torch_cuda, T):
    """Afterstates with 16, 18, 24 and 30 chance items: on the 16 lanes of a direction at depth 2 lanes take a second item
    (none, two, eight, all but two of them); on the 4 lanes at depth 1 up to eight."""
    rnet = random_net(TUPLES_8x4[:T], 92)
    want_2, trace = search_ref(WIDE_FANS, 2, rnet)
    assert max(trace.root_items) == 30 and {16, 18, 24, 30} <= set(trace.root_items) and trace.negative_inexact > 0
    want_1, trace_1 = search_ref(WIDE_FANS, 1, rnet)
    assert trace_1.root_items == trace.root_items
    check_both_forms(g, torch_cuda, WIDE_FANS, rnet, searches=[(2, want_2), (1, want_1)])


# ------------------------------------------------------------------------------------ 3. values at their stated bounds
def bound_boards(n, seed, max_empty):
    """Exponents 14..17 (they merge: a 16 + 16 scores 2^17) with 0..max_empty empty cells."""
    rng = np.random.default_rng(seed)
    b = rng.integers(14, 18, size=(n, 16)).astype(np.uint8)
    for x in b:
        x[rng.choice(16, int(rng.integers(0, max_empty + 1)), replace=False)] = 0
    return b


# a full board whose move left leaves one empty cell where a spawned 2 ends the game, while up and down keep the pair of 1s:
# under all-INT32_MIN weights left is worth about -2^37 / 10 and up about -2^37; and the same board turned by a quarter
_DEAD_END = np.array([1, 1, 3, 2, 5, 6, 3, 4, 1, 2, 8, 5, 4, 5, 6, 7], np.uint8)
DEAD_ENDS = np.stack([_DEAD_END, np.rot90(_DEAD_END.reshape(4, 4)).reshape(16)])


# equal to its transpose: up and left are worth the same, down and right too, so the largest value is shared at any depth
MIRRORED = np.array([[16, 0, 15, 14, 0, 17, 14, 16, 15, 14, 16, 15, 14, 16, 15, 17]], np.uint8)


def bound_case(kind, F):
    rnet = ref.Net(TUPLES_8x4, F)
    rnet.weights[:] = bound_fill(kind, rnet.weights.shape)
    shallow_b = np.concatenate([bound_boards(20, 94, 10), np.array([[16, 16, 3, 0, 0, 2, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0]], np.uint8),
                                symmetric_boards(), DEAD_ENDS])
    deep_b = np.concatenate([bound_boards(4, 95, 2), MIRRORED, DEAD_ENDS])
    return (rnet, shallow_b, deep_b, ref.evaluate_batch(shallow_b, rnet), ref.values_batch(shallow_b, rnet),
            search_ref(shallow_b, 1, rnet), search_ref(deep_b, 2, rnet))


def symmetric_boards():
    """Boards equal to their mirror images: the eight look-ups of a tuple coincide, so under weights of +-2^31 at random V
    is a few large terms and spreads far from 0."""
    rng = np.random.default_rng(96)
    out = []
    for _ in range(40):
        q = rng.choice(np.array([0, 14, 15, 16, 17]), size=(2, 2))
        half = np.concatenate([q, q[:, ::-1]], 1)
        out.append(np.concatenate([half, half[::-1]]).reshape(16))
    return np.array(out, np.uint8)


def ties(value):
    """Rows whose largest legal value two directions share."""
    legal = value != ref.ILLEGAL
    top = np.where(legal, value, ref.ILLEGAL).max(1, keepdims=True)
    return legal.any(1) & (((value == top) & legal).sum(1) > 1)


def far_apart(value):
    """Rows with legal values on both sides of -2^36: further apart than a key bias below the stated 2^48 would order."""
    legal = value != ref.ILLEGAL
    return ((value < -(1 << 36)) & legal).any(1) & ((value >= -(1 << 36)) & legal).any(1)


@pytest.mark.parametrize("F", [0, 16])
@pytest.mark.parametrize("kind", ["min", "max", "random"])
def test_values_at_the_stated_bounds(g, torch_cuda, kind, F):
    """T = 8, L = 4 with every weight INT32_MIN, every weight INT32_MAX, or one of the two at random: |V| reaches 2^37, a
    gain of 2^17 at F = 16 adds 2^33, and every value stays inside the 2^50 the key's bias relies on."""
    rnet, shallow_b, deep_b, want_e, want_v, (want_1, trace_1), (want_2, trace_2) = cached(("bound", kind, F), lambda: bound_case(kind, F))
    gains = [ref.move(ref.plain(b), d)[1] for b in shallow_b for d in range(4)]
    assert max(gains) >= 1 << 17 and (want_e[0] != ref.ILLEGAL).all(1).any() and ((deep_b == 0).sum(1) <= 2).all()
    for value in (want_e[0], want_1[1], want_2[1]):
        legal = value != ref.ILLEGAL
        assert legal.any() and (np.abs(value[legal]) < 1 << 50).all()
    if kind == "min":
        assert want_v.min() == -(1 << 37) == want_e[4][(want_e[0] != ref.ILLEGAL).any(1)].min()
        assert far_apart(want_1[1]).any() and far_apart(want_2[1]).any()
    if kind == "max":
        assert (want_e[0] > 1 << 37).any() and (want_1[1] > 1 << 37).any() and (want_2[1] > 1 << 37).any()
    if kind in ("min", "max"):   # root ties, broken to the smallest direction
        for act, value in ((want_e[1], want_e[0]), want_1, want_2):
            rows = ties(value)
            assert rows.any() and (act[rows] == np.where(value[rows] != ref.ILLEGAL, value[rows], ref.ILLEGAL).argmax(1)).all()
        assert trace_1.root_ties > 0 and trace_2.root_ties > 0
    if kind == "random":
        assert trace_1.negative_inexact > 0 and trace_2.negative_inexact > 0
        assert want_v.min() < -(1 << 36) and want_v.max() > 1 << 35      # V of both signs, far from 0
    check_both_forms(g, torch_cuda, shallow_b, rnet, want_e, want_v, [(1, want_1)])
    check_both_forms(g, torch_cuda, deep_b, rnet, searches=[(2, want_2)])


# ------------------------------------------------------------------------------------ 4. ragged n
@pytest.mark.parametrize("n", [1, 3, 5, 17, 65])
def test_ragged_batches_write_nothing_past_n(g, torch_cuda, n):
    """Fewer boards than a wave holds (16 in evaluate, 4 at depth 1, 1 at depth 2) and counts that leave one partly
    filled: the n rows equal the reference, the 512 elements after them keep their fill.  Row i is base row i mod m."""
    torch = torch_cuda
    T = 3
    net = device_net(g, net_of(T))
    want_e, _, (want_1, _) = shallow(T)
    base_2 = [0, 1, 2, 10, 11]
    want_2 = tuple(w[base_2] for w in deep(T)[0])

    def over(shape, dtype):
        size = int(np.prod(shape))
        buf = torch.full((size + 512,), 0x5A, dtype=dtype, device="cuda")
        return buf, buf[:size].view(shape)

    def run(names, shapes, base, want, launch):
        bufs = {f: over(shapes[f], torch.uint8 if f in ("action", "after") else torch.int64) for f in names}
        launch(dev(torch, base[np.arange(n) % len(base)]), [bufs[f][1] for f in names])
        for k, f in enumerate(names):
            assert_rows_periodic(torch, bufs[f][1], dev(torch, want[k]), 1 << 20)
            assert bool((bufs[f][0][int(np.prod(shapes[f])):] == 0x5A).all()), (f, "written past n")

    eval_shapes = {"value": (n, 4), "action": (n,), "best": (n,), "after": (n, 16), "after_value": (n,)}
    run(EVAL_NAMES, eval_shapes, boards_64(), want_e, lambda d, out: net.evaluate(d, out=g.NTupleEval(*out)))
    run(SEARCH_NAMES, eval_shapes, boards_64(), want_1, lambda d, out: net.search(d, 1, out=g.NTupleSearch(*out)))
    run(SEARCH_NAMES, eval_shapes, near_full_12()[base_2], want_2, lambda d, out: net.search(d, 2, out=g.NTupleSearch(*out)))
