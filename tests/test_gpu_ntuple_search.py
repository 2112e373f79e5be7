"""GPU: the n-tuple expectimax kernel (g2048_ntuple_search, g2048_ntuple_search_plain) and
record_search(player="ntuple", net_depth=1) equal the pure-Python reference tests/ntuple_search_ref.py bit for bit.
Every test shows from the reference (never from the code under test) that its input reaches the edge it names.
"""
import ctypes as C

import numpy as np
import pytest

import ntuple_ref as ref
import ntuple_search_ref as sref
from analysis_helpers import (ONE_LEGAL, SEARCH_MAX_LANES, TERMINAL, assert_rows_periodic, g, mid_game, mixed_boards,  # noqa: F401 (g: fixture)
                              tiled)
from ntuple_helpers import TUPLES_2x6, TUPLES_17x4, random_net
from ntuple_search_helpers import PAIR_ONLY, SEARCH_GROUP, SEARCH_NAMES, assert_search_equal

pytestmark = pytest.mark.gpu


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


TIES = np.array([[0] * 5 + [3] + [0] * 10, [1, 1] + [0] * 14], np.uint8)   # every move alike; right and left mirror images
_cases = {}


def case(name):
    """(boards, depth, reference network, the reference's (action, value), its trace), computed once per case."""
    if name not in _cases:
        tuples, seed, depth = {"17x4": (TUPLES_17x4, 21, 1), "2x6": (TUPLES_2x6, 22, 1), "depth2": (TUPLES_17x4, 23, 2)}[name]
        if depth == 1:
            boards = np.concatenate([mixed_boards(245, seed), TIES, PAIR_ONLY, ONE_LEGAL, TERMINAL])
            boards[5::7] += (32 * (boards[5::7] > 0)).astype(np.uint8)   # exponents are read mod 32
            boards[3::11, [0, 6, 9, 15]] = [15, 16, 17, 31]             # at and past the clamp
        else:
            boards = np.concatenate([mid_game(38, seed, max_empty=2), PAIR_ONLY, TERMINAL])
        rnet, trace = random_net(tuples, seed), sref.Trace()
        _cases[name] = boards, depth, rnet, sref.search_batch(boards, depth, rnet, trace), trace
    return _cases[name]


@pytest.mark.parametrize("name", ["17x4", "2x6", "depth2"])
def test_search_equals_the_reference(g, torch_cuda, name):
    torch = torch_cuda
    boards, depth, rnet, want, trace = case(name)
    legal = want[1] != sref.ILLEGAL
    assert trace.negative_inexact > 20 and trace.terminal_children >= 2 and not legal[-1].any() and (~legal).any()
    assert (want[1][legal] < 0).any() and (want[1][legal] > 0).any() and len(set(want[0].tolist())) == 4
    if depth == 1:
        assert trace.root_ties >= 2 and (want[0] != ref.greedy_actions(boards, rnet)).any()   # look-ahead changes the move
    net = device_net(g, rnet)
    d = dev(torch, boards)
    assert_search_equal(to_np(net.search(d, depth)), want, boards, "plain")
    assert_search_equal(to_np(net.search(d.view(-1, 4, 4), depth)), want, boards, "plain [n, 4, 4]")
    # the engine form, with scores set so that the deficit bits of the records are populated
    eng = g.Batched2048(len(boards), seed=3)
    try:
        eng.set_boards(boards % 32)
        eng.set_scores(np.random.default_rng(1).integers(1, 1 << 24, len(boards)).astype(np.int32))
        rec = eng.records().clone()
        assert bool((rec[:, 8:] > 31).any())
        clock, stats = eng.clock, eng.episode_stats()
        assert_search_equal(to_np(eng.ntuple_search(net, depth)), want, boards, "engine")
        assert torch.equal(eng.records(), rec) and eng.clock == clock and eng.episode_stats() == stats
    finally:
        eng.close()


def test_out_single_fields_and_no_output(g, torch_cuda):
    torch = torch_cuda
    boards, depth, rnet, want, _ = case("17x4")
    n = len(boards)
    net, d = device_net(g, rnet), dev(torch, boards)
    shapes = {"action": ((n,), torch.uint8), "value": ((n, 4), torch.int64)}
    eng = g.Batched2048(n)
    try:
        eng.set_boards(boards % 32)
        for k, name in enumerate(SEARCH_NAMES):
            for form in ("plain", "engine"):
                shape, dtype = shapes[name]
                buf = torch.full((int(np.prod(shape)) + 512,), 0x5A, dtype=dtype, device="cuda")   # nothing past n is written
                out = g.NTupleSearch(*[buf[:int(np.prod(shape))].view(shape) if f == name else None for f in SEARCH_NAMES])
                res = net.search(d, depth, out=out) if form == "plain" else eng.ntuple_search(net, depth, out=out)
                assert all((r is None) == (f != name) for f, r in zip(SEARCH_NAMES, res)) and res[k] is out[k]
                assert np.array_equal(res[k].cpu().numpy(), want[k]), (name, form)
                assert bool((buf[int(np.prod(shape)):] == 0x5A).all()), (name, form)
        with pytest.raises(ValueError, match="no output"):
            net.search(d, out=g.NTupleSearch(None, None))
        from gym2048_amd import _lib
        lib, io = _lib.load(), _lib.NTupleSearchIO(1)
        assert lib.g2048_ntuple_search(eng._h, C.byref(net._c), C.byref(io), None) == -1
        assert b"requests no output" in lib.g2048_last_error()
        assert lib.g2048_ntuple_search_plain(d.data_ptr(), n, C.byref(net._c), C.byref(io), None) == -1
        assert b"requests no output" in lib.g2048_last_error()
    finally:
        eng.close()


def test_grid_stride_passes(g, torch_cuda):
    """n * G lanes past the grid cap: the boards after the first pass are reached by the kernel's stride loop.  The
    periodic base's own rows come from a launch of the base alone (no stride), itself pinned to the reference on every
    eighth row; the other cases of this module pin whole batches."""
    torch = torch_cuda
    n, m = SEARCH_MAX_LANES // SEARCH_GROUP[1] + 1027, 509
    assert SEARCH_GROUP[1] * n > SEARCH_MAX_LANES and n % m != 0
    rnet = random_net(TUPLES_17x4, 31)
    base = mixed_boards(m, 32)
    net = device_net(g, rnet)
    want = net.search(dev(torch, base), 1)
    assert_search_equal([w[::8] for w in to_np(want)], sref.search_batch(base[::8], 1, rnet), base[::8], "base")
    got = net.search(tiled(torch, base, n).contiguous(), 1)
    for k in range(2):
        assert_rows_periodic(torch, got[k], want[k], 1 << 20)


def test_plain_rows_on_a_side_stream(g, torch_cuda):
    torch = torch_cuda
    boards, depth, rnet, want, _ = case("2x6")
    net, d = device_net(g, rnet), dev(torch, boards)
    first = net.search(d, depth)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        src = torch.empty_like(d)
        torch.cuda._sleep(1 << 20)           # the copy below lands late: a search on another stream would see garbage
        src.copy_(d)
        got = net.search(src, depth)
    torch.cuda.synchronize()
    assert torch.equal(got.action, first.action) and torch.equal(got.value, first.value)
    assert_search_equal(to_np(got), want, boards, "side stream")


def test_record_search_ntuple_depth_1(g, torch_cuda):
    """The CSV of record_search(player="ntuple", net_depth=1) equals, byte for byte, the reference-format writer
    (Transitions.export_csv, pinned to the reference's bytes by tests/test_transitions.py) fed the reference player's
    game; on some of those boards the greedy player (net_depth=0) would have moved otherwise."""
    from gym2048_amd.transitions import Transitions
    n, k, seed = 16, 12, 5
    rnet = random_net(TUPLES_17x4, 51, lo=-(1 << 16), hi=1 << 16)
    rows = {f: [] for f in ("x", "action", "reward", "next_x", "done")}
    greedy_differs = 0
    for env in ref.make_envs(n, seed):                      # env-major rows
        for _ in range(k):
            rows["x"].append(list(env.M))
            action = sref.search(ref.env_board(env), 1, rnet)[1]
            greedy_differs += action != ref.evaluate(ref.env_board(env), rnet)[1]
            reward, done, _, _ = env.step(action)
            rows["action"].append(action), rows["reward"].append(reward), rows["next_x"].append(list(env.M)), rows["done"].append(done)
            if done:
                env.reset()
    want = Transitions(rows["x"], rows["action"], rows["reward"], rows["next_x"], rows["done"])
    assert greedy_differs > 0
    net = device_net(g, rnet)
    eng = g.Batched2048(n, seed=seed)
    try:
        eng.reset()
        got = Transitions.record_search(eng, k, player="ntuple", net=net, net_depth=1)
    finally:
        eng.close()
    assert got.to_csv_text() == want.to_csv_text()
