"""GPU: the n-tuple reduced search kernel (g2048_ntuple_reduced_search), one workgroup per board, the children
of a 4 spawn searched reduce4 plies shallower.  Constant schedules 0..4 and one mixed launch against the host build of the
definition (tests/host_ntuple_reduced, itself checked against the pure-Python reference on the CPU); depth 0 and 1 against
evaluate and search(1) on the GPU, bit for bit; depth 2..4 against one chance level composed in Python integers over the GPU's own
lower depths; the engine form, the mask, the outputs left out; every tuple count; and the game report of ReducedPlayer against
the move-by-move composition.  Expected values never come from the call under test at the depth under test."""
import numpy as np
import pytest

from analysis_helpers import ONE_LEGAL, TERMINAL, g  # noqa: F401 (g: fixture)
from ntuple_adaptive_helpers import (CRAFTED, ILLEGAL, MIXED_SCHEDULE, SKIPPED, adaptive_np, constant, crafted_net, empties_boards,
                                     named_boards, rows_at)
from ntuple_deep_helpers import FAMILIES, LOW_STAGE, cached, dev, dev_u32, device_net, engine_with, family_net, mixed_net, staged_net
from ntuple_reduced_helpers import REDUCE4, TIED, compose_reduced, composed_game, host_root, load_host_reduced
from ntuple_search_helpers import PAIR_ONLY, assert_search_equal

pytestmark = pytest.mark.gpu
NETS = {"uniform": crafted_net, "staged": staged_net, "mixed": mixed_net}        # mixed: the "4x6+4x4"-shaped network
DEPTH4_MAX_EMPTY = 8      # the host build's depth 4 of a board with more empty cells takes seconds: those run under MIXED_SCHEDULE


def late_boards():
    return np.concatenate([CRAFTED, named_boards(), LOW_STAGE, PAIR_ONLY, TERMINAL, ONE_LEGAL, TIED])


def boards_at(depth):
    """About 40 boards: the late boards and one board per empty-cell count (up to DEPTH4_MAX_EMPTY at depth 4)."""
    e = empties_boards()
    return np.concatenate([late_boards(), e if depth < 4 else e[:DEPTH4_MAX_EMPTY + 1]])


def expected(kind, depth, R, boards, key):
    """(action, value) by the host build's recursion of the definition, once per process."""
    return cached(("reduced gpu expected", kind, depth, R, key), lambda: host_root(load_host_reduced(), boards, depth, R, NETS[kind]()))


def both_forms(g, net, boards, schedule, R, check):
    """check(form, (action, value, depth) as numpy) for the plain form and for an engine whose records hold ``boards``."""
    import torch
    check("plain", adaptive_np(net.reduced_search(dev(torch, boards), schedule, R)))
    eng = engine_with(g, boards)
    try:
        assert bool((eng.records()[:, 8:] > 31).any()), "inputs: the score-deficit bits are populated"
        check("engine", adaptive_np(eng.ntuple_reduced_search(net, schedule, R)))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 1. constant schedules
@pytest.mark.parametrize("kind", list(NETS))
@pytest.mark.parametrize("R", REDUCE4)
@pytest.mark.parametrize("depth", range(5))
def test_a_constant_schedule_equals_the_host_build(g, torch_cuda, depth, R, kind):
    boards = boards_at(depth)
    assert 25 <= len(boards) <= 45
    want = expected(kind, depth, R, boards, "set")
    legal = want[1] != ILLEGAL
    assert legal.any(1).sum() >= 24 and (~legal).all(1).sum() >= 2, "inputs: live and dead boards"
    net = device_net(g, NETS[kind]())

    def check(form, got):
        assert_search_equal(got[:2], want, boards, f"{kind}, depth {depth}, R {R}, {form}")
        assert (got[2] == depth).all(), "the depth output is the schedule's depth"
    both_forms(g, net, boards, constant(depth), R, check)


@pytest.mark.parametrize("R", REDUCE4)
def test_a_launch_of_one_board(g, torch_cuda, R):
    torch = torch_cuda
    net = device_net(g, crafted_net())
    for depth in range(5):
        want = expected("uniform", depth, R, CRAFTED[2:3], "one")
        got = adaptive_np(net.reduced_search(dev(torch, CRAFTED[2:3]), constant(depth), R))
        assert_search_equal(got[:2], want, CRAFTED[2:3], f"n = 1, depth {depth}, R {R}")
        assert got[2].tolist() == [depth]


@pytest.mark.parametrize("kind", list(NETS))
@pytest.mark.parametrize("R", REDUCE4)
def test_one_launch_mixes_every_depth(g, torch_cuda, R, kind):
    torch = torch_cuda
    boards = empties_boards()
    rows, depths = rows_at(MIXED_SCHEDULE, boards)
    assert sorted(rows) == [0, 1, 2, 3, 4] and (boards[rows[4]] == 0).sum(1).max() <= DEPTH4_MAX_EMPTY
    want = (np.zeros(17, np.uint8), np.zeros((17, 4), np.int64))
    for depth, at in rows.items():
        want[0][at], want[1][at] = expected(kind, depth, R, boards[at], "mixed")
    net = device_net(g, NETS[kind]())

    def check(form, got):
        assert_search_equal(got[:2], want, boards, f"{kind}, R {R}, {form}")
        assert got[2].tolist() == list(MIXED_SCHEDULE)
        assert got[0][16] == 0 and (got[1][16] == ILLEGAL).all(), "the all-empty board is dead"
    both_forms(g, net, boards, MIXED_SCHEDULE, R, check)
    got = adaptive_np(net.reduced_search(dev(torch, boards[::-1]), MIXED_SCHEDULE, R))
    assert_search_equal(tuple(x[::-1] for x in got[:2]), want, boards, f"{kind}, reversed")


# ------------------------------------------------------------------------------------------------ 2. the identities
@pytest.mark.parametrize("kind", list(NETS))
@pytest.mark.parametrize("R", REDUCE4)
def test_depth_0_and_1_are_evaluate_and_search_1(g, torch_cuda, R, kind):
    torch = torch_cuda
    boards = boards_at(0)
    net, d = device_net(g, NETS[kind]()), dev(torch, boards)
    ev = net.evaluate(d)
    s1 = net.search(d, 1)
    for depth, want in ((0, (ev.action.cpu().numpy(), ev.value.cpu().numpy())), (1, (s1.action.cpu().numpy(), s1.value.cpu().numpy()))):
        got = adaptive_np(net.reduced_search(d, constant(depth), R))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), f"{kind}, depth {depth}, R {R}: not bit-equal"


@pytest.mark.parametrize("kind", list(NETS))
@pytest.mark.parametrize("R", REDUCE4)
@pytest.mark.parametrize("depth", [2, 3, 4])
def test_one_chance_level_composed_over_gpu_calls(g, torch_cuda, depth, R, kind):
    """The 2 children at depth D - 1 and the 4 children at max(D - 1 - R, 0), their values from the GPU: this call at the lower
    constant depths, evaluate and search(1) at depth 0 and 1."""
    torch = torch_cuda
    rnet, boards = NETS[kind](), named_boards()
    net = device_net(g, rnet)

    def state_values(kids, k):
        d = dev(torch, kids)
        if k == 0:
            return net.evaluate(d).value.cpu().numpy()
        if k == 1:
            return net.search(d, 1).value.cpu().numpy()
        return net.reduced_search(d, constant(k), R).value.cpu().numpy()

    want, dead = compose_reduced(boards, rnet.frac_bits, depth, R, state_values)
    legal = want[1] != ILLEGAL
    assert len(boards) == 9 and dead >= 1 and legal[:8].any(1).all() and not legal[8].any() and (np.abs(want[1][legal]) < 1 << 50).all()

    def check(form, got):
        assert_search_equal(got[:2], want, boards, f"{kind}, depth {depth}, R {R}, {form}")
    both_forms(g, net, boards, constant(depth), R, check)


# ------------------------------------------------------------------------------------------------ 3. the mask, the outputs
@pytest.mark.parametrize("R", REDUCE4)
def test_mask(g, torch_cuda, R):
    torch = torch_cuda
    boards = empties_boards()[:16]
    net = device_net(g, staged_net())
    n = len(boards)
    want = adaptive_np(net.reduced_search(dev(torch, boards), MIXED_SCHEDULE, R))
    assert (want[1] != ILLEGAL).any(1).all(), "inputs: every board has a legal move"
    eng = engine_with(g, boards)
    try:
        plain = adaptive_np(eng.ntuple_reduced_search(net, MIXED_SCHEDULE, R))
        assert all(np.array_equal(a, b) for a, b in zip(plain, want)), "the engine form equals the plain form"
        on = adaptive_np(eng.ntuple_reduced_search(net, MIXED_SCHEDULE, R, active=dev_u32(torch, np.full(n, 7))))
        assert all(np.array_equal(a, b) for a, b in zip(on, want))
        off = adaptive_np(eng.ntuple_reduced_search(net, MIXED_SCHEDULE, R, active=dev_u32(torch, np.zeros(n))))
        assert (off[0] == 0).all() and (off[1] == ILLEGAL).all() and (off[2] == SKIPPED).all()
        for flip in (0, 1):
            m = np.arange(n) % 2 == flip
            words = np.array([1, 1 << 31, 0xffffffff, 7], np.uint32)[np.arange(n) % 4]
            alt = adaptive_np(eng.ntuple_reduced_search(net, MIXED_SCHEDULE, R, active=dev_u32(torch, np.where(m, words, 0))))
            assert_search_equal((alt[0][m], alt[1][m]), (want[0][m], want[1][m]), boards[m], f"masked, flip {flip}")
            assert np.array_equal(alt[2][m], want[2][m])
            assert (alt[0][~m] == 0).all() and (alt[1][~m] == ILLEGAL).all() and (alt[2][~m] == SKIPPED).all()
    finally:
        eng.close()


def test_out_fields_left_none_are_not_written_and_the_engine_is_untouched(g, torch_cuda):
    torch = torch_cuda
    boards = empties_boards()
    net = device_net(g, crafted_net())
    n = len(boards)
    d = dev(torch, boards)
    want = adaptive_np(net.reduced_search(d, MIXED_SCHEDULE, 1))
    eng = engine_with(g, boards)
    try:
        for form in ("plain", "engine", "masked"):
            act = torch.full((n + 512,), 0x5A, dtype=torch.uint8, device="cuda")
            dep = torch.full((n + 512,), 0x5A, dtype=torch.uint8, device="cuda")
            val = torch.full((4 * n + 512,), 0x5A5A, dtype=torch.int64, device="cuda")
            call = {"plain": lambda out: net.reduced_search(d, MIXED_SCHEDULE, 1, out=out),
                    "engine": lambda out: eng.ntuple_reduced_search(net, MIXED_SCHEDULE, 1, out=out),
                    "masked": lambda out: eng.ntuple_reduced_search(net, MIXED_SCHEDULE, 1, out=out, active=dev_u32(torch, np.ones(n)))}[form]
            res = call(g.NTupleAdaptive(act[:n], None, None))
            assert res.value is None and res.depth is None and np.array_equal(res.action.cpu().numpy(), want[0]), form
            assert bool((act[n:] == 0x5A).all()) and bool((val == 0x5A5A).all()) and bool((dep == 0x5A).all()), form
            act.fill_(0x5A)
            res = call(g.NTupleAdaptive(None, val[:4 * n].view(n, 4), None))
            assert res.action is None and res.depth is None and np.array_equal(res.value.cpu().numpy(), want[1]), form
            assert bool((val[4 * n:] == 0x5A5A).all()) and bool((dep == 0x5A).all()) and bool((act == 0x5A).all()), form
            val.fill_(0x5A5A)
            res = call(g.NTupleAdaptive(act[:n], None, dep[:n]))
            assert res.value is None and np.array_equal(res.depth.cpu().numpy(), want[2]) and np.array_equal(res.action.cpu().numpy(), want[0]), form
            assert bool((dep[n:] == 0x5A).all()) and bool((act[n:] == 0x5A).all()) and bool((val == 0x5A5A).all()), form
        rec, clock, stats = eng.records().clone(), eng.clock, eng.episode_stats()
        for R in REDUCE4:
            eng.ntuple_reduced_search(net, "4-ply-late", R)
        assert torch.equal(eng.records(), rec) and eng.clock == clock and eng.episode_stats() == stats, "the engine's state is untouched"
    finally:
        eng.close()


def test_active_on_a_plain_form_and_a_bad_reduction_are_refused(g, torch_cuda):
    import ctypes as C
    from gym2048_amd import ntuple
    torch = torch_cuda
    net = device_net(g, crafted_net())
    d = dev(torch, empties_boards())
    io, out = ntuple._adaptive_io(len(d), d.device, MIXED_SCHEDULE, None, dev_u32(torch, np.ones(len(d))), reduce4=1)
    out.action.fill_(0x5A)
    with pytest.raises(g.G2048Error, match="plain form"):
        net._launch(net._fn("reduced_search_plain"), d, net._ref(d.device), C.byref(io))
    io, out2 = ntuple._adaptive_io(len(d), d.device, MIXED_SCHEDULE, out, reduce4=1)
    io.reduce4 = 0
    with pytest.raises(g.G2048Error, match="g2048_ntuple_adaptive_search"):
        net._launch(net._fn("reduced_search_plain"), d, net._ref(d.device), C.byref(io))
    torch.cuda.synchronize()
    assert bool((out.action == 0x5A).all()), "nothing was launched"


# ------------------------------------------------------------------------------------------------ 4. every tuple count
@pytest.mark.parametrize("family, T", [(f, T) for f, Ts in FAMILIES.items() for T in Ts])
def test_every_tuple_count_at_depth_3(g, torch_cuda, family, T):
    """One (family, T) = three kernels: plain boards, engine records, engine records with a mask; one depth-3, R = 1 launch each."""
    torch = torch_cuda
    rnet = family_net(family, T)
    net = device_net(g, rnet)
    boards = np.concatenate([empties_boards()[:7], CRAFTED, TIED, TERMINAL])
    want = cached(("reduced gpu family", family, T), lambda: host_root(load_host_reduced(), boards, 3, 1, rnet))
    assert (want[1][1:-1] != ILLEGAL).any(1).all() and (want[1][-1] == ILLEGAL).all()

    def check(form, got):
        assert_search_equal(got[:2], want, boards, f"{family} T={T}, {form}")
        assert (got[2] == 3).all()
    both_forms(g, net, boards, constant(3), 1, check)
    eng = engine_with(g, boards)
    try:
        m = np.arange(len(boards)) % 3 != 1
        got = adaptive_np(eng.ntuple_reduced_search(net, constant(3), 1, active=dev_u32(torch, m)))
        assert_search_equal((got[0][m], got[1][m]), (want[0][m], want[1][m]), boards[m], f"{family} T={T}, masked")
        assert np.array_equal(got[2], np.where(m, 3, SKIPPED))
        assert (got[0][~m] == 0).all() and (got[1][~m] == ILLEGAL).all()
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 5. games
def recording(g, net, schedule, R):
    """A ReducedPlayer that keeps the actions it chose, one uint8 [n] array per move."""
    class Recording(g.ReducedPlayer):
        def __call__(self, engine, actions, active=None):
            super().__call__(engine, actions, active=active)
            self.actions.append(actions.cpu().numpy().copy())
    player = Recording(net, schedule, R)
    player.actions = []
    return player


# the deep end of a rule at the START of a game, where eight boards afford it: 4-ply on a board of two tiles, 3-ply on three
OPENING_SCHEDULE = (0,) + (1,) * 11 + (2, 3, 4, 4, 4)


@pytest.mark.parametrize("R", REDUCE4)
def test_play_games_with_the_reduced_player_is_the_composition(g, torch_cuda, R):
    """play_games(player=ReducedPlayer(net, schedule, R)) against ntuple_reduced_search(active=games left) -> play_step, call by
    call, on a second engine with the same seed: eight fresh boards; actions, hist, moves and the return sum."""
    torch = torch_cuda
    net = device_net(g, crafted_net())
    steps = 24
    a, b = g.Batched2048(8, seed=11), g.Batched2048(8, seed=11)
    try:
        player = recording(g, net, OPENING_SCHEDULE, R)
        report = g.play_games(a, net, 1, chunk=8, max_steps=steps, player=player)
        want = composed_game(torch, b, net, OPENING_SCHEDULE, R, steps)
        assert len({tuple(r) for r in want.actions.T.tolist()}) > 1, "inputs: the boards do not all play the same moves"
        assert set(want.depths.ravel().tolist()) - {SKIPPED} >= {1, 2, 3, 4}, "inputs: the depths the boards are searched at"
        assert np.array_equal(np.array(player.actions), want.actions), "the actions, move by move"
        assert report.games == want.played and report.unfinished == 8 - want.played and report.moves == want.moves
        assert report.hist == want.hist and report.mean_score == (want.return_sum / want.played if want.played else 0.0)
        assert torch.equal(a.records(), b.records()) and a.clock == b.clock and a.episode_stats() == b.episode_stats()
    finally:
        a.close(), b.close()
