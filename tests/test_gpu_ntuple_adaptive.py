"""GPU: the n-tuple adaptive search kernel (g2048_ntuple_adaptive_search), one workgroup per board at a depth
chosen from the board's own empty cells.  Constant schedules 0..3 against the existing calls, bit for bit (evaluate, search,
deep_search); depth 4 against the pure-Python reference on three crafted boards and against the definition composed from
deep_search(depth=3) of the children; one launch that mixes every depth; the mask; every instantiation of the kernel; and the
game report of AdaptivePlayer against the move-by-move composition.  Expected values never come from the code under test."""
import numpy as np
import pytest

from analysis_helpers import TERMINAL, g  # noqa: F401 (g: fixture)
from ntuple_adaptive_helpers import (CRAFTED, ILLEGAL, MIXED_SCHEDULE, SKIPPED, adaptive_np, composed_depth_4, composed_game, constant,
                                     crafted_net, crafted_reference, empties_boards, existing_calls, expected_mixed, named_boards, rows_at)
from ntuple_deep_helpers import FAMILIES, LOW_STAGE, dev, dev_u32, device_net, engine_with, family_net, mixed_net, near_full, staged_net
from ntuple_helpers import TUPLES_8x4, random_net
from ntuple_search_helpers import WIDE_FANS, assert_search_equal

pytestmark = pytest.mark.gpu
NETS = {"uniform": lambda: random_net(TUPLES_8x4[:1], 41), "staged": staged_net, "mixed": mixed_net}
_nets = {}


def rnet_of(kind):
    if kind not in _nets:
        _nets[kind] = NETS[kind]()
    return _nets[kind]


def both_forms(g, net, boards, schedule, check):
    """check(form, (action, value, depth) as numpy) for the plain form and for an engine whose records hold ``boards``."""
    import torch
    check("plain", adaptive_np(net.adaptive_search(dev(torch, boards), schedule)))
    eng = engine_with(g, boards)
    try:
        assert bool((eng.records()[:, 8:] > 31).any()), "inputs: the score-deficit bits are populated"
        check("engine", adaptive_np(eng.ntuple_adaptive_search(net, schedule)))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 1. constant schedules
@pytest.mark.parametrize("kind", list(NETS))
@pytest.mark.parametrize("depth", [0, 1, 2, 3])
def test_a_constant_schedule_gives_the_bits_of_the_existing_calls(g, torch_cuda, depth, kind):
    torch = torch_cuda
    boards = np.concatenate([near_full(2)[0], WIDE_FANS, LOW_STAGE, TERMINAL])
    assert len(boards) == 19 and (boards == 0).sum(1).max() == 15
    rnet = rnet_of(kind)
    net = device_net(g, rnet)
    calls = existing_calls(net, dev(torch, boards), depth)
    assert [name for name, _ in calls] == {0: ["evaluate"], 1: ["search(1)"], 2: ["search(2)", "deep_search(2)"], 3: ["deep_search(3)"]}[depth]
    legal = calls[0][1][1] != ILLEGAL
    assert legal[:18].any(1).all() and not legal[18].any(), "inputs: only TERMINAL is dead"

    def check(form, got):
        for name, want in calls:
            assert_search_equal(got[:2], want, boards, f"{kind}, depth {depth}, {form} vs {name}")
        assert (got[2] == depth).all()
    both_forms(g, net, boards, constant(depth), check)


# ------------------------------------------------------------------------------------------------ 2. depth 4
def test_depth_4_equals_the_reference(g, torch_cuda):
    """(a) tests/ntuple_search_ref.py at depth 4 on the three crafted boards."""
    want = crafted_reference()
    assert (want[1] != ILLEGAL).sum(1).tolist() == [2, 2, 3]
    net = device_net(g, crafted_net())

    def check(form, got):
        assert_search_equal(got[:2], want, CRAFTED, form)
        assert (got[2] == 4).all()
    both_forms(g, net, CRAFTED, constant(4), check)


@pytest.mark.parametrize("kind", list(NETS))
def test_depth_4_equals_the_composition_of_depth_3_calls(g, torch_cuda, kind):
    torch = torch_cuda
    rnet, boards = rnet_of(kind), named_boards()
    net = device_net(g, rnet)
    want = composed_depth_4(torch, net, rnet, boards)
    legal = want[1] != ILLEGAL
    assert len(boards) == 9 and legal[:8].any(1).all() and not legal[8].any() and (np.abs(want[1][legal]) < 1 << 50).all()

    def check(form, got):
        assert_search_equal(got[:2], want, boards, f"{kind}, {form}")
        assert (got[2] == 4).all()
    both_forms(g, net, boards, constant(4), check)


# ------------------------------------------------------------------------------------------------ 3. one mixed launch
@pytest.mark.parametrize("kind", list(NETS))
def test_one_launch_mixes_every_depth(g, torch_cuda, kind):
    torch = torch_cuda
    rnet, boards = rnet_of(kind), empties_boards()
    net = device_net(g, rnet)
    want = expected_mixed(torch, net, rnet, boards, MIXED_SCHEDULE)
    assert want[2].tolist() == list(MIXED_SCHEDULE) and sorted(set(MIXED_SCHEDULE)) == [0, 1, 2, 3, 4]
    assert (want[1][:16] != ILLEGAL).any(1).all(), "inputs: every board but the empty one has a legal move"

    def check(form, got):
        assert_search_equal(got[:2], want[:2], boards, f"{kind}, {form}")
        assert got[2].tolist() == list(MIXED_SCHEDULE)
        assert got[0][16] == 0 and (got[1][16] == ILLEGAL).all() and got[2][16] == MIXED_SCHEDULE[16], "the all-empty board is dead"
    both_forms(g, net, boards, MIXED_SCHEDULE, check)
    # the same boards in reverse order: a workgroup's table does not care what it held
    got = adaptive_np(net.adaptive_search(dev(torch, boards[::-1]), MIXED_SCHEDULE))
    assert_search_equal(tuple(x[::-1] for x in got[:2]), want[:2], boards, f"{kind}, reversed")


# ------------------------------------------------------------------------------------------------ 4. the mask, the outputs
def test_mask(g, torch_cuda):
    torch = torch_cuda
    rnet, boards = rnet_of("staged"), empties_boards()[:16]
    net = device_net(g, rnet)
    n = len(boards)
    eng = engine_with(g, boards)
    try:
        want = adaptive_np(eng.ntuple_adaptive_search(net, MIXED_SCHEDULE))
        assert (want[1] != ILLEGAL).any(1).all(), "inputs: every board has a legal move"
        on = adaptive_np(eng.ntuple_adaptive_search(net, MIXED_SCHEDULE, active=dev_u32(torch, np.full(n, 7))))
        assert all(np.array_equal(a, b) for a, b in zip(on, want))
        off = adaptive_np(eng.ntuple_adaptive_search(net, MIXED_SCHEDULE, active=dev_u32(torch, np.zeros(n))))
        assert (off[0] == 0).all() and (off[1] == ILLEGAL).all() and (off[2] == SKIPPED).all()
        for flip in (0, 1):
            m = np.arange(n) % 2 == flip
            words = np.array([1, 1 << 31, 0xffffffff, 7], np.uint32)[np.arange(n) % 4]
            active = dev_u32(torch, np.where(m, words, 0))
            alt = adaptive_np(eng.ntuple_adaptive_search(net, MIXED_SCHEDULE, active=active))
            assert_search_equal((alt[0][m], alt[1][m]), (want[0][m], want[1][m]), boards[m], f"masked, flip {flip}")
            assert np.array_equal(alt[2][m], want[2][m])
            assert (alt[0][~m] == 0).all() and (alt[1][~m] == ILLEGAL).all() and (alt[2][~m] == SKIPPED).all()
    finally:
        eng.close()


def test_active_on_a_plain_form_is_refused(g, torch_cuda):
    """NTupleNet.adaptive_search has no ``active``; the library's plain form, called as the wrapper calls it, refuses one."""
    import ctypes as C
    from gym2048_amd import ntuple
    torch = torch_cuda
    net = device_net(g, rnet_of("uniform"))
    d = dev(torch, empties_boards())
    io, out = ntuple._adaptive_io(len(d), d.device, MIXED_SCHEDULE, None, dev_u32(torch, np.ones(len(d))))
    out.action.fill_(0x5A)
    with pytest.raises(g.G2048Error, match="plain form"):
        net._launch(net._fn("adaptive_search_plain"), d, net._ref(d.device), C.byref(io))
    torch.cuda.synchronize()
    assert bool((out.action == 0x5A).all()), "nothing was launched"


def test_misaligned_active_and_value_are_refused_by_the_engine_form(g, torch_cuda):
    """The engine form with a live engine: ``active`` 2 bytes and ``value`` 8 bytes off their alignment (addresses inside real
    buffers; torch has no such views, so the struct is filled as the wrapper fills it and the address moved)."""
    import ctypes as C
    from gym2048_amd import ntuple
    from gym2048_amd._lib import check
    torch = torch_cuda
    net = device_net(g, rnet_of("uniform"))
    boards = empties_boards()
    n = len(boards)
    eng = engine_with(g, boards)
    try:
        active = dev_u32(torch, np.ones(n + 1))
        value = torch.empty((n + 1, 4), dtype=torch.int64, device="cuda")
        for field, shift, words in (("active", 2, ("misaligned", "active", "4 bytes")), ("value", 8, ("misaligned", "value", "16 bytes"))):
            io, out = ntuple._adaptive_io(n, eng.device, MIXED_SCHEDULE, (torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda"), value[:n], None),
                                          active[:n])
            setattr(io, field, getattr(io, field) + shift)
            with pytest.raises(g.G2048Error) as err:
                check(net._fn("adaptive_search")(eng._h, net._ref(eng.device), C.byref(io), eng._stream()))
            assert all(w in str(err.value) for w in words), str(err.value)
            torch.cuda.synchronize()
            assert bool((out.action == 0x5A).all()), "nothing was launched"
    finally:
        eng.close()


def test_out_fields_left_none_are_not_written(g, torch_cuda):
    torch = torch_cuda
    rnet, boards = rnet_of("uniform"), empties_boards()
    net = device_net(g, rnet)
    n = len(boards)
    d = dev(torch, boards)
    want = adaptive_np(net.adaptive_search(d, MIXED_SCHEDULE))
    eng = engine_with(g, boards)
    try:
        for form in ("plain", "engine", "masked"):
            act = torch.full((n + 512,), 0x5A, dtype=torch.uint8, device="cuda")
            dep = torch.full((n + 512,), 0x5A, dtype=torch.uint8, device="cuda")
            val = torch.full((4 * n + 512,), 0x5A5A, dtype=torch.int64, device="cuda")
            call = {"plain": lambda out: net.adaptive_search(d, MIXED_SCHEDULE, out=out),
                    "engine": lambda out: eng.ntuple_adaptive_search(net, MIXED_SCHEDULE, out=out),
                    "masked": lambda out: eng.ntuple_adaptive_search(net, MIXED_SCHEDULE, out=out, active=dev_u32(torch, np.ones(n)))}[form]
            res = call(g.NTupleAdaptive(act[:n], None, None))
            assert res.value is None and res.depth is None and np.array_equal(res.action.cpu().numpy(), want[0]), form
            assert bool((act[n:] == 0x5A).all()) and bool((val == 0x5A5A).all()) and bool((dep == 0x5A).all()), form
            act.fill_(0x5A)
            res = call(g.NTupleAdaptive(None, val[:4 * n].view(n, 4), dep[:n]))
            assert res.action is None and np.array_equal(res.value.cpu().numpy(), want[1]) and np.array_equal(res.depth.cpu().numpy(), want[2]), form
            assert bool((val[4 * n:] == 0x5A5A).all()) and bool((dep[n:] == 0x5A).all()) and bool((act == 0x5A).all()), form
        rec, clock, stats = eng.records().clone(), eng.clock, eng.episode_stats()
        eng.ntuple_adaptive_search(net, "4-ply-late")
        assert torch.equal(eng.records(), rec) and eng.clock == clock and eng.episode_stats() == stats, "the engine's state is untouched"
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 5. every instantiation
INSTANCE_SCHEDULE = (4, 4, 4, 3, 2, 2, 1, 1, 0) + (0,) * 8     # every depth among boards of at most 8 empty cells; CRAFTED at depth 4


@pytest.mark.parametrize("family, T", [(f, T) for f, Ts in FAMILIES.items() for T in Ts])
def test_every_instantiation(g, torch_cuda, family, T):
    """One (family, T) = three kernels: plain boards, engine records, engine records with a mask."""
    torch = torch_cuda
    rnet = family_net(family, T)
    net = device_net(g, rnet)
    boards = np.concatenate([empties_boards()[:9], CRAFTED])
    rows, depths = rows_at(INSTANCE_SCHEDULE, boards)
    assert sorted(rows) == [0, 1, 2, 3, 4] and depths[-3:].tolist() == [4, 4, 4] and len(rows[4]) == 6
    want = expected_mixed(torch, net, rnet, boards, INSTANCE_SCHEDULE)
    assert (want[1] != ILLEGAL).any(1).all()

    def check(form, got):
        assert_search_equal(got[:2], want[:2], boards, f"{family} T={T}, {form}")
        assert np.array_equal(got[2], depths)
    both_forms(g, net, boards, INSTANCE_SCHEDULE, check)
    eng = engine_with(g, boards)
    try:
        m = np.arange(len(boards)) % 3 != 1
        got = adaptive_np(eng.ntuple_adaptive_search(net, INSTANCE_SCHEDULE, active=dev_u32(torch, m)))
        assert_search_equal((got[0][m], got[1][m]), (want[0][m], want[1][m]), boards[m], f"{family} T={T}, masked")
        assert np.array_equal(got[2], np.where(m, depths, SKIPPED))
        assert (got[0][~m] == 0).all() and (got[1][~m] == ILLEGAL).all()
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 6. games
def recording(g, net, schedule):
    """An AdaptivePlayer that keeps the actions it chose, one uint8 [n] array per move."""
    class Recording(g.AdaptivePlayer):
        def __call__(self, engine, actions, active=None):
            super().__call__(engine, actions, active=active)
            self.actions.append(actions.cpu().numpy().copy())
    player = Recording(net, schedule)
    player.actions = []
    return player


# the deep end of a rule at the START of a game, where eight boards afford it: 4-ply on a board of two tiles, 3-ply on three
OPENING_SCHEDULE = (0,) + (1,) * 11 + (2, 3, 4, 4, 4)


@pytest.mark.parametrize("schedule, steps, depths", [("4-ply-late", 40, {1, 2}), (OPENING_SCHEDULE, 24, {1, 2, 3, 4})],
                         ids=["4-ply-late", "opening"])
def test_play_games_with_the_adaptive_player_is_the_composition(g, torch_cuda, schedule, steps, depths):
    """play_games(player=AdaptivePlayer(net, schedule)) against ntuple_adaptive_search(active=games left) -> play_step, call by
    call, on a second engine with the same seed: eight fresh boards; actions, hist, moves and the return sum.  Fresh boards do
    not reach the deep end of "4-ply-late" in 40 moves (asserted from the composition's depth output), so a second rule puts
    its depths 3 and 4 where a game begins."""
    torch = torch_cuda
    net = device_net(g, rnet_of("uniform"))
    a, b = g.Batched2048(8, seed=11), g.Batched2048(8, seed=11)
    try:
        player = recording(g, net, schedule)
        report = g.play_games(a, net, 1, chunk=8, max_steps=steps, player=player)
        want = composed_game(torch, b, net, schedule, steps)
        assert len({tuple(r) for r in want.actions.T.tolist()}) > 1, "inputs: the boards do not all play the same moves"
        assert set(want.depths.ravel().tolist()) - {SKIPPED} >= depths, "inputs: the depths the boards are searched at"
        assert np.array_equal(np.array(player.actions), want.actions), "the actions, move by move"
        assert report.games == want.played and report.unfinished == 8 - want.played and report.moves == want.moves
        assert report.hist == want.hist and report.mean_score == (want.return_sum / want.played if want.played else 0.0)
        assert torch.equal(a.records(), b.records()) and a.clock == b.clock and a.episode_stats() == b.episode_stats()
    finally:
        a.close(), b.close()
