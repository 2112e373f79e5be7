"""GPU: the n-tuple network kernels (g2048_ntuple_evaluate, _evaluate_plain, _values_plain, _update_plain), the TD(0)
trainer built on them and record_search(player="ntuple") equal the pure-Python reference tests/ntuple_ref.py bit for bit.
Every test shows from the reference (never from the code under test) that its input reaches the edge it names.

Figures measured on the MI355X: profiles/r11_ntuple_probe.txt."""
import ctypes as C

import numpy as np
import pytest

import ntuple_ref as ref
from analysis_helpers import (ONE_LEGAL, SEARCH_MAX_LANES, TERMINAL, assert_rows_periodic, g, mixed_boards,  # noqa: F401 (g: fixture)
                              random_boards, tiled)
from ntuple_helpers import EVAL_NAMES, TUPLES_2x6, TUPLES_8x6, TUPLES_17x4, assert_eval_equal, random_net

pytestmark = pytest.mark.gpu

INT32_MAX, INT32_MIN = (1 << 31) - 1, -(1 << 31)


def device_net(g, rnet):
    """An NTupleNet on the GPU with the shape and weights of a reference network."""
    import torch
    net = g.NTupleNet(rnet.tuples, frac_bits=rnet.frac_bits, device="cuda:0")
    net.weights.copy_(torch.as_tensor(rnet.weights.astype(np.int32)))
    return net


def dev(torch, a):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda:0")


def to_np(e):
    return tuple(None if t is None else t.cpu().numpy() for t in e)


_cases = {}


def case(name):
    """(boards, reference network, the reference's evaluate and values), computed once per shape."""
    if name not in _cases:
        tuples, seed = {"17x4": (TUPLES_17x4, 21), "2x6": (TUPLES_2x6, 22)}[name]
        boards = np.concatenate([mixed_boards(2003, seed), ONE_LEGAL, TERMINAL])
        boards[5::7] += (32 * (boards[5::7] > 0)).astype(np.uint8)   # exponents are read mod 32
        boards[3::11, [0, 6, 9, 15]] = [15, 16, 17, 31]   # at and past the clamp
        rnet = random_net(tuples, seed)
        _cases[name] = boards, rnet, ref.evaluate_batch(boards, rnet), ref.values_batch(boards, rnet)
    return _cases[name]


@pytest.mark.parametrize("name", ["17x4", "2x6"])
def test_evaluate_and_values_equal_the_reference(g, torch_cuda, name):
    torch = torch_cuda
    boards, rnet, want, want_v = case(name)
    legal = want[0] != ref.ILLEGAL
    assert (want[0][legal] < 0).any() and (want[0][legal] > 0).any() and len(set(want[1].tolist())) == 4 and not legal[-1].any()
    net = device_net(g, rnet)
    d = dev(torch, boards)
    assert_eval_equal(to_np(net.evaluate(d)), want, boards, "plain")
    assert np.array_equal(net.values(d).cpu().numpy(), want_v)
    assert np.array_equal(net.values(d.view(-1, 4, 4)).cpu().numpy(), want_v)
    # the engine form, with scores set so that the deficit bits of the records are populated
    eng = g.Batched2048(len(boards), seed=3)
    try:
        eng.set_boards(boards % 32)
        eng.set_scores(np.random.default_rng(1).integers(1, 1 << 24, len(boards)).astype(np.int32))
        rec = eng.records().clone()
        assert bool((rec[:, 8:] > 31).any())
        clock, stats = eng.clock, eng.episode_stats()
        assert_eval_equal(to_np(eng.ntuple_evaluate(net)), want, boards, "engine")
        assert torch.equal(eng.records(), rec) and eng.clock == clock and eng.episode_stats() == stats
    finally:
        eng.close()


def test_out_single_fields_and_no_output(g, torch_cuda):
    torch = torch_cuda
    boards, rnet, want, _ = case("17x4")
    n = len(boards)
    net, d = device_net(g, rnet), dev(torch, boards)
    shapes = {"value": ((n, 4), torch.int64), "action": ((n,), torch.uint8), "best": ((n,), torch.int64),
              "after": ((n, 16), torch.uint8), "after_value": ((n,), torch.int64)}
    eng = g.Batched2048(n)
    try:
        eng.set_boards(boards % 32)
        for k, name in enumerate(EVAL_NAMES):
            for form in ("plain", "engine"):
                shape, dtype = shapes[name]
                buf = torch.full((int(np.prod(shape)) + 512,), 0x5A, dtype=dtype, device="cuda")   # nothing past n is written
                out = g.NTupleEval(*[buf[:int(np.prod(shape))].view(shape) if f == name else None for f in EVAL_NAMES])
                res = net.evaluate(d, out=out) if form == "plain" else eng.ntuple_evaluate(net, out=out)
                assert all((r is None) == (f != name) for f, r in zip(EVAL_NAMES, res)) and res[k] is out[k]
                assert np.array_equal(res[k].cpu().numpy(), want[k]), (name, form)
                assert bool((buf[int(np.prod(shape)):] == 0x5A).all()), (name, form)
        with pytest.raises(ValueError, match="no output"):
            net.evaluate(d, out=g.NTupleEval(None, None, None, None, None))
        from gym2048_amd import _lib
        lib, io = _lib.load(), _lib.NTupleIO()
        assert lib.g2048_ntuple_evaluate(eng._h, C.byref(net._c), C.byref(io), None) == -1
        assert b"requests no output" in lib.g2048_last_error()
        assert lib.g2048_ntuple_evaluate_plain(d.data_ptr(), n, C.byref(net._c), C.byref(io), None) == -1
        assert b"requests no output" in lib.g2048_last_error()
    finally:
        eng.close()


def test_grid_stride_passes(g, torch_cuda):
    """4n lanes past the grid cap: the boards after the first pass are reached by the kernel's stride loop."""
    torch = torch_cuda
    n, m = SEARCH_MAX_LANES // 4 + 1027, 509
    assert 4 * n > SEARCH_MAX_LANES and n % m != 0
    rnet = random_net(TUPLES_17x4, 31)
    base = mixed_boards(m, 32)
    want = [dev(torch, w) for w in ref.evaluate_batch(base, rnet)]
    net = device_net(g, rnet)
    got = net.evaluate(tiled(torch, base, n).contiguous())
    for k in range(5):
        assert_rows_periodic(torch, got[k], want[k], 1 << 20)
    v = net.values(tiled(torch, base, n).contiguous())
    assert_rows_periodic(torch, v, dev(torch, ref.values_batch(base, rnet)), 1 << 20)


def check_update(g, torch, rnet, boards, deltas, lr_shift):
    """device == reference for one update launch; returns (the new weights, the reference's trace)."""
    after, trace = rnet.copy(), {}
    ref.update(after, boards, deltas, lr_shift, trace)
    net = device_net(g, rnet)
    net.update(dev(torch, np.asarray(boards, np.uint8).reshape(-1, 16)), dev(torch, np.asarray(deltas, np.int64)), lr_shift)
    got = net.weights.cpu().numpy().astype(np.int64)
    bad = np.argwhere(got != after.weights)
    assert len(bad) == 0, f"{len(bad)} weights differ, first {bad[0].tolist()}: {got[tuple(bad[0])]} vs {after.weights[tuple(bad[0])]}"
    return after.weights, trace


def test_update_edges(g, torch_cuda):
    """The edge cases of tests/test_ntuple_host.py on the device."""
    torch = torch_cuda
    small = random_net(TUPLES_17x4, 10, lo=-1000, hi=1000)
    # negative deltas with a shift that floors; zero steps touch nothing
    assert [ref.step_of(d, 1) for d in (-5, 5, -1, 1)] == [-3, 2, -1, 0]
    _, trace = check_update(g, torch, small, random_boards(8, 11), [-5, 5, -1, 1, -7, 0, -(1 << 20) - 1, 3], 1)
    assert trace["zero"] == 2 and trace["sat"] == 0
    _, trace = check_update(g, torch, small, random_boards(3, 12), [-1, -(1 << 40) - 1, 1 << 39], 40)
    assert trace["zero"] == 1
    # saturation at both int32 ends: 2^31 is the first step to clip, -2^31 the last to fit
    _, trace = check_update(g, torch, ref.Net(TUPLES_2x6, 10), random_boards(4, 12), [1 << 40, -(1 << 40), (1 << 31) << 7, -(1 << 31) << 7], 7)
    assert trace["sat"] == 3
    # a weight at INT32_MAX wraps
    top = ref.Net(TUPLES_17x4, 10)
    top.weights[:] = INT32_MAX
    new, trace = check_update(g, torch, top, random_boards(1, 13), [1], 0)
    assert trace["wrap"] > 0 and new.min() <= INT32_MIN + 8
    # duplicate boards in one batch
    b = random_boards(3, 15)
    new, _ = check_update(g, torch, small, np.concatenate([b, b[:1], b[:1], b[1:2]]), [64, -128, 192, 64, 640, 256], 6)
    once = small.copy()
    ref.update(once, b, [12, 2, 3], 0)
    assert np.array_equal(new, once.weights)
    # T = 1, L = 1 and T = 8, L = 6: the last entry of the last table
    for tuples in (((9,),), TUPLES_8x6):
        rnet = random_net(tuples, 16)
        T, size = len(tuples), 16 ** len(tuples[0])
        boards = np.concatenate([np.array([[15, 16, 17, 31] * 4], np.uint8), random_boards(20, 17)])
        hits = []
        ref.value(ref.plain(boards[0]), rnet, hits)
        assert (T - 1, size - 1) in hits
        net = device_net(g, rnet)
        assert_eval_equal(to_np(net.evaluate(dev(torch, boards))), ref.evaluate_batch(boards, rnet), boards, T)
        new, _ = check_update(g, torch, rnet, boards, np.arange(1, 22) * 1000, 3)
        assert new[T - 1, size - 1] != rnet.weights[T - 1, size - 1]


def test_update_same_address_contention_and_split_launches(g, torch_cuda):
    torch = torch_cuda
    # 4 096 copies of one board, step 1: every touched weight = count x multiplicity
    board = np.array([[1, 2, 0, 0, 2, 1, 0, 0, 0, 0, 3, 0, 0, 0, 0, 3]], np.uint8)   # equal to its transpose: entries read twice
    rnet = ref.Net(TUPLES_17x4, 10)
    hits = []
    ref.value(ref.plain(board), rnet, hits)
    assert len(set(hits)) < len(hits)
    net = device_net(g, rnet)
    net.update(dev(torch, np.repeat(board, 4096, axis=0)), torch.ones(4096, dtype=torch.int64, device="cuda"), 0)
    got = net.weights.cpu().numpy()
    want = np.zeros_like(got)
    for t, i in hits:
        want[t, i] += 4096
    assert np.array_equal(got, want) and want.max() >= 2 * 4096
    # two disjoint half-batches in two launches == one launch
    rnet = random_net(TUPLES_2x6, 41, lo=-(1 << 20), hi=1 << 20)
    boards = mixed_boards(3001, 42)
    deltas = np.random.default_rng(43).integers(-(1 << 30), 1 << 30, len(boards))
    want, _ = check_update(g, torch, rnet, boards, deltas, 9)
    net = device_net(g, rnet)
    d, dl = dev(torch, boards), dev(torch, deltas)
    net.update(d[1500:].contiguous(), dl[1500:].contiguous(), 9)
    net.update(d[:1500].contiguous(), dl[:1500].contiguous(), 9)
    assert np.array_equal(net.weights.cpu().numpy().astype(np.int64), want)


def test_update_grid_stride_passes(g, torch_cuda):
    """n lanes past the grid cap: the boards after the first pass are reached by the kernel's stride loop.  Only the last
    pass and one board of the first have a delta, so the reference stays small."""
    torch = torch_cuda
    n, m = SEARCH_MAX_LANES + 1027, 509
    assert n > SEARCH_MAX_LANES and n % m != 0
    base = mixed_boards(m, 111)
    live = np.concatenate([[5], np.arange(SEARCH_MAX_LANES, n)])
    values = np.random.default_rng(112).integers(-(1 << 24), 1 << 24, len(live))
    values[values == 0] = 1
    rnet = random_net(TUPLES_17x4, 113, lo=-(1 << 20), hi=1 << 20)
    net = device_net(g, rnet)
    trace = {}
    ref.update(rnet, base[live % m], values, 2, trace)
    assert len(live) == 1028 and trace.get("zero", 0) < len(live) // 2
    deltas = torch.zeros(n, dtype=torch.int64, device="cuda")
    deltas[dev(torch, live)] = dev(torch, values)
    net.update(tiled(torch, base, n).contiguous(), deltas, 2)
    got = net.weights.cpu().numpy().astype(np.int64)
    bad = np.argwhere(got != rnet.weights)
    assert len(bad) == 0, f"{len(bad)} weights differ, first {bad[0].tolist()}: {got[tuple(bad[0])]} vs {rnet.weights[tuple(bad[0])]}"


# lr_shift 4: of the shifts 0, 2, 4, 6, 8, 12 the one at which the reference trainer finishes episodes within the 40 steps
# (the large steps drive weights to the int32 ends and the play turns erratic); the test asserts it from the reference
TRAIN = dict(n=64, steps=40, seed=42, lr_shift=4)


@pytest.fixture(scope="module")
def trained():
    """The reference trainer on oracle.cpu_ref boards: (network, boards, scores, trace), once for the module."""
    rnet, trace = ref.Net(TUPLES_17x4, 10), {}
    envs = ref.make_envs(TRAIN["n"], TRAIN["seed"])
    for _ in range(TRAIN["steps"]):
        ref.td_step(envs, rnet, TRAIN["lr_shift"], trace)
    return rnet, np.array([ref.env_board(e) for e in envs], np.uint8), np.array([e.score for e in envs]), trace


def test_train_equals_the_reference_trainer(g, torch_cuda, trained):
    torch = torch_cuda
    rnet, boards, scores, trace = trained
    assert (rnet.weights != 0).any() and trace["episodes"] >= 1
    net = g.NTupleNet("17x4", frac_bits=10)
    eng = g.Batched2048(TRAIN["n"], seed=TRAIN["seed"])
    try:
        eng.reset()
        assert g.train(eng, net, TRAIN["steps"], TRAIN["lr_shift"]) is net
        torch.cuda.synchronize()
        assert np.array_equal(net.weights.cpu().numpy().astype(np.int64), rnet.weights)
        assert np.array_equal(eng.get_boards().reshape(-1, 16), boards) and np.array_equal(eng.get_scores(), scores)
        assert eng.episode_stats()["episodes"] == trace["episodes"]
    finally:
        eng.close()


def test_two_shards_sharing_the_weights_equal_the_unsharded_run(g, torch_cuda, trained):
    from gym2048_amd.ntuple import td_evaluate, td_update, td_work
    torch = torch_cuda
    rnet, boards, scores, _ = trained
    net = g.NTupleNet("17x4", frac_bits=10)
    cut = 24
    a, b = g.Batched2048(cut, seed=TRAIN["seed"]), g.Batched2048(TRAIN["n"] - cut, seed=TRAIN["seed"], board_offset=cut)
    try:
        works = [td_work(e) for e in (a, b)]
        for e in (a, b):
            e.reset()
        for _ in range(TRAIN["steps"]):
            for e, w in zip((a, b), works):     # every shard evaluates under the step's weights ...
                td_evaluate(e, net, w)
            for w in works:                     # ... before any shard updates them
                td_update(net, w, TRAIN["lr_shift"])
        torch.cuda.synchronize()
        assert np.array_equal(net.weights.cpu().numpy().astype(np.int64), rnet.weights)
        assert np.array_equal(np.concatenate([a.get_boards(), b.get_boards()]).reshape(-1, 16), boards)
        assert np.array_equal(np.concatenate([a.get_scores(), b.get_scores()]), scores)
    finally:
        a.close()
        b.close()


def test_record_search_ntuple(g, torch_cuda):
    """The CSV of record_search(player="ntuple") equals, byte for byte, the reference-format writer (Transitions.export_csv,
    pinned to the reference's bytes by tests/test_transitions.py) fed the reference player's game."""
    from gym2048_amd.transitions import Transitions
    n, k, seed = 16, 12, 5
    rnet = random_net(TUPLES_17x4, 51, lo=-(1 << 16), hi=1 << 16)
    rows = {f: [] for f in ("x", "action", "reward", "next_x", "done")}
    for env in ref.make_envs(n, seed):                      # env-major rows
        for _ in range(k):
            rows["x"].append(list(env.M))
            action = ref.evaluate(ref.env_board(env), rnet)[1]
            reward, done, _, _ = env.step(action)
            rows["action"].append(action), rows["reward"].append(reward), rows["next_x"].append(list(env.M)), rows["done"].append(done)
            if done:
                env.reset()
    want = Transitions(rows["x"], rows["action"], rows["reward"], rows["next_x"], rows["done"])
    assert len(set(rows["action"])) == 4
    eng = g.Batched2048(n, seed=seed)
    try:
        eng.reset()
        got = Transitions.record_search(eng, k, player="ntuple", net=device_net(g, rnet))
    finally:
        eng.close()
    assert got.to_csv_text() == want.to_csv_text()
