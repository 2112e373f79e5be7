"""GPU: the episode books behind g2048_stats at their carry, borrow and width edges.

A wavefront's slot keeps four 64-bit counters as eight dwords; a step launch stores the three low counter dwords and
the high ones only when they change, each of the five flushing kernels sums what it flushes its own way, adjust_slot
adds a SIGNED delta, clear_stats rewrites whole slots, and the two readers (stats_kernel + stats_merge_kernel, and the
one-launch returns_summary_kernel) sum 64-bit values through narrower pieces.  Ordinary play never gets near any of
those edges, so here the state is planted through the checkpoint blob (tests/episode_slots.py) and every expected
value comes from the C oracle's books or from integer arithmetic on what was planted.  Every comparison is exact.
"""
import numpy as np
import pytest

from episode_slots import (EP, GAIN, ILL, PEND, StateBlob, books_return_sum, check_slots_match_stats, n_slots, n_waves,
                           slot_sums)

pytestmark = pytest.mark.gpu
M32 = 1 << 32
MASK32 = np.uint64(0xFFFFFFFF)


def _readers(eng):
    """Both readers; the returns-only summary must agree with the full reduction on what it computes."""
    from gym2048_amd.batched import parse_stats
    full = eng.episode_stats()
    summary = parse_stats(eng.episode_stats_device(returns_only=True))
    for key in ("episodes", "illegal_ends", "return_sum"):
        assert summary[key] == full[key], (key, summary[key], full[key])
    return full


def _per_slot(x, n):
    pad = np.zeros(n_waves(n) * 64, np.int64)
    pad[:n] = x
    return pad.reshape(-1, 64).sum(axis=1)


def _pending_words(pending, n):
    pad = np.zeros(n_waves(n) * 64, np.uint64)
    pad[:n] = pending
    return (pad.reshape(-1, 64) << np.arange(64, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)


# ---------------------------------------------------------------------------------------------------- carry matrix
# form -> what runs: g2048_step (step_kernel / step_numpy_kernel), g2048_rollout by per-step launches (the same kernels,
# a launch train, a cached graph or two chains), g2048_rollout_fused with actions and per-step outputs (rollout_fused_kernel
# / rollout_fused_numpy_kernel), g2048_rollout_random (rollout_random_kernel / the fused numpy kernel); always auto-reset
FORMS = ("step", "rollout", "fused", "random")
CASES = [(f, m, a) for f in FORMS for m in ("philox", "numpy") for a in ((1,) if f == "random" else (1, 0))]


def _carry_case(torch, n, form, mode, auto_reset, k=27, chains=1, graph=False):
    from gym2048_amd.batched import Batched2048
    from oracle import OracleBatch
    seed = 1000 + n + 7 * FORMS.index(form) + (1 if mode == "numpy" else 0)
    eng = Batched2048(n, seed=seed, rng=mode, chains=chains)
    ora = OracleBatch(n, seed)
    numpy_mode = mode == "numpy"
    if numpy_mode:
        ora.seed_numpy(seed)
    ora_step = ora.step_numpy if numpy_mode else ora.step
    eng.reset()
    ora.reset_numpy() if numpy_mode else ora.reset()
    for _ in range(6):                                       # non-zero counters and scores before anything is planted
        eng.step(None, auto_reset=bool(auto_reset), want_info=False)
        ora_step(None, auto_reset=bool(auto_reset))
    assert np.array_equal(eng.get_boards().reshape(n, 16), ora.boards)
    blob = check_slots_match_stats(eng)                      # the helper's offsets are the engine's

    # ---- dry run of the oracle: every slot's increments over the k steps, and the per-step outputs
    synthetic = form in ("step", "random")
    acts = None if synthetic else np.random.default_rng(seed).integers(0, 4, (k, n), dtype=np.uint8)
    ep0, ret0, fin0 = int(ora.ep_count.sum()), ora.return_sum, ora.finished_return_sum
    inc_ep, inc_ill, inc_g = (np.zeros(n, np.int64) for _ in range(3))
    outs = {key: np.zeros((k, n), dt) for key, dt in (("reward", np.float32), ("terminated", np.uint8),
                                                      ("illegal", np.uint8), ("highest", np.uint8))}
    for j in range(k):
        ora_step(None if synthetic else acts[j], auto_reset=bool(auto_reset))
        done, illegal = ora.terminated.astype(bool), ora.illegal.astype(bool)
        inc_ep += done
        inc_ill += done & illegal
        inc_g += np.where(illegal, 0, ora.reward.astype(np.int64))   # an illegal move scores nothing
        for key in outs:
            outs[key][j] = getattr(ora, key)
    assert int(inc_ep.sum()) == int(ora.ep_count.sum()) - ep0
    nw, ns = n_waves(n), n_slots(n)
    inc = np.stack([_per_slot(inc_ep, n), _per_slot(inc_ill, n), _per_slot(inc_g, n)], axis=1).astype(np.uint64)

    # ---- plant: slot s lands exactly ON 2^32 in counter c where bit c of s % 8 is set, one count short elsewhere;
    # every third slot starts with non-zero high dwords; the padding slots of a ragged batch hold values nobody may add
    s = np.arange(nw)
    want = ((s[:, None] % 8) >> np.arange(3)[None, :]) & 1 == 1
    lo = np.where(want & (inc > 0), np.uint64(M32) - inc, np.uint64(M32 - 1) - inc)
    hi = np.where((s % 3 == 1)[:, None], (1 + s % 11)[:, None] + np.arange(3)[None, :], 0).astype(np.uint64)
    c = blob.counters()
    c[:nw, :3] = (hi << np.uint64(32)) | lo
    junk = np.array([(5 << 32) | 0xFFFFFFF0, (6 << 32) | 0xFFFFFFFF, (7 << 32) | 0xFFFFFFFE, 0], np.uint64)
    c[nw:] = junk
    blob.set_counters(c)
    blob.load_into(eng)
    planted = c.copy()
    ep, ill, g = slot_sums(planted, n)
    st0 = _readers(eng)
    assert (st0["episodes"], st0["illegal_ends"]) == (ep, ill)
    assert st0["return_sum"] == books_return_sum(g, eng.get_scores(), blob.pending())

    # ---- the engine plays the same k steps
    dev = eng.device
    graphs0 = eng.graph_replays
    if form == "step":
        for j in range(k):
            r, t = eng.step(None, auto_reset=bool(auto_reset), want_info=False)
            assert np.array_equal(r.cpu().numpy(), outs["reward"][j]), j
            assert np.array_equal(t.cpu().numpy(), outs["terminated"][j]), j
        got = {}
    elif form == "random":
        eng.rollout_random(k)
        got = {}
    elif form == "rollout":
        got = {"reward": torch.zeros((k, n), dtype=torch.float32, device=dev),
               "terminated": torch.zeros((k, n), dtype=torch.uint8, device=dev)}
        plan = eng.prepare_rollout(torch.as_tensor(acts, device=dev), auto_reset=bool(auto_reset), **got)
        if graph:
            plan.prepare_graph()
        plan.run()
    else:
        got = {key: torch.zeros((k, n), dtype=torch.float32 if key == "reward" else torch.uint8, device=dev) for key in outs}
        eng.rollout(torch.as_tensor(acts.astype(np.int64), device=dev), auto_reset=bool(auto_reset), fused=True, **got)
    if graph:
        assert eng.graph_replays == graphs0 + 1, eng.graph_status
    if chains == 2:
        assert eng.chains_used == 2
    for key, buf in got.items():
        assert np.array_equal(buf.cpu().numpy(), outs[key]), key
    assert np.array_equal(eng.get_boards().reshape(n, 16), ora.boards)
    assert np.array_equal(eng.get_scores(), ora.score)

    # ---- every slot moved by exactly the oracle's increments; the high dwords changed exactly where they must
    after = StateBlob(eng)
    got_c = after.counters()
    expect = planted.copy()
    expect[:nw, :3] += inc
    expect[:nw, PEND] = _pending_words(ora.pending, n)
    carried = (expect[:nw, :3] >> np.uint64(32)) != (planted[:nw, :3] >> np.uint64(32))
    assert np.array_equal(carried, want & (inc > 0))
    for cnt in range(3):                                     # the inputs reach the edge in every combination that matters
        others = np.delete(carried, cnt, axis=1).any(axis=1)
        assert (carried[:, cnt] & ~others).any(), f"no slot carries in counter {cnt} alone"
        assert ((expect[:nw, cnt] & MASK32) == 0)[carried[:, cnt]].all()
        assert ((expect[:nw, cnt] & MASK32) == MASK32)[~carried[:, cnt]].any()
    bad = np.nonzero((got_c[:nw] != expect[:nw]).any(axis=1))[0]
    assert bad.size == 0, f"slots {bad[:8]}: got {got_c[bad[:2]]}, want {expect[bad[:2]]}"
    assert np.array_equal(after.slots[nw:ns], blob.slots[nw:ns]), "a padding slot was written"

    # ---- both readers: the absolute books, and the oracle's deltas
    st1 = _readers(eng)
    ep1, ill1, g1 = slot_sums(expect, n)
    assert (st1["episodes"], st1["illegal_ends"]) == (ep1, ill1)
    assert st1["return_sum"] == books_return_sum(g1, ora.score, ora.pending)
    assert st1["episodes"] - st0["episodes"] == int(ora.ep_count.sum()) - ep0
    assert st1["illegal_ends"] - st0["illegal_ends"] == int(inc_ill.sum())
    assert st1["return_sum"] - st0["return_sum"] == ora.return_sum - ret0
    if auto_reset:
        assert st1["return_sum"] - st0["return_sum"] == ora.finished_return_sum - fin0


@pytest.mark.parametrize("n", [4133, 5017])                  # ragged for 64 and for 512: padding slots behind the last wave
@pytest.mark.parametrize("form,mode,auto_reset", CASES)
def test_every_flushing_kernel_carries_into_the_high_dwords(torch_cuda, n, form, mode, auto_reset):
    """Slots planted exactly one step's worth below 2^32 (and one count further down) in every combination of the three
    counters: each kernel that flushes a slot must store the high dwords where a counter carries and nowhere else, and
    both readers must then report exactly the oracle's books."""
    _carry_case(torch_cuda, n, form, mode, auto_reset)


def test_two_chain_rollout_carries(torch_cuda):
    """The same with the batch split over two launch chains (g2048_set_chains(2))."""
    _carry_case(torch_cuda, 5017, "rollout", "philox", 1, k=70, chains=2)


def test_cached_graph_rollout_carries(torch_cuda):
    """The same with the rollout replayed from the engine's cached hipGraph (step_graph_kernel)."""
    _carry_case(torch_cuda, 4133, "rollout", "philox", 0, graph=True)


# ------------------------------------------------------------------------------------- borrow (adjust_slot), clear
def _plant_gain_edges(eng, ora, delta):
    """Plant G = 2^32 + x in every slot so that adding `delta` (signed, per slot) crosses a 2^32 boundary exactly in
    the even slots (a borrow to high dword 0, or a carry to 2) and stops one short of it in the odd ones.  The oracle's
    books move by the same amount.  Returns the expected G after the call and where its high dword must leave 1."""
    n = eng.n_envs
    nw = n_waves(n)
    blob = StateBlob(eng)
    c = blob.counters()
    edge = np.arange(nw) % 2 == 0
    mag = np.abs(delta)
    x = np.where(delta < 0, np.where(edge, mag - 1, mag), np.where(edge, M32 - mag, M32 - mag - 1))
    x = np.where(delta == 0, 12345, x).astype(np.int64)
    assert (x >= 0).all() and (x < M32).all()
    new = (M32 + x).astype(np.uint64)
    ora.gain_total += int(new.sum(dtype=np.uint64)) - int(c[:nw, GAIN].sum(dtype=np.uint64))
    c[:nw, GAIN] = new
    blob.set_counters(c)
    blob.load_into(eng)
    assert _readers(eng)["return_sum"] == ora.return_sum
    crossing = edge & (delta != 0)
    assert crossing.sum() > nw // 4 and (~crossing).any()
    return (M32 + x + delta).astype(np.uint64), crossing


def _check_gain(eng, ora, expect_g, crossing):
    """G is exactly `expect_g`, its high dword left 1 exactly where `crossing` says, and both readers give the
    oracle's return_sum."""
    n = eng.n_envs
    g = StateBlob(eng).counters()[: n_waves(n), GAIN]
    assert np.array_equal(g, expect_g)
    assert np.array_equal((g >> np.uint64(32)) != 1, crossing)
    assert np.array_equal(eng.get_scores(), ora.score)
    assert _readers(eng)["return_sum"] == ora.return_sum


def test_reset_and_set_scores_borrow_and_seed_clears_high_dwords(torch_cuda):
    """adjust_slot adds a signed delta: a masked reset that abandons running episodes, one that also clears pending
    marks, and score imports that lower and raise scores (host and device buffers) must borrow from and carry into the
    high dword of G exactly where the arithmetic says.  Then g2048_seed on slots with four non-zero high dwords must
    leave whole zero high halves: the statistics of a fresh engine holding the same boards."""
    torch = torch_cuda
    from gym2048_amd.batched import Batched2048
    from oracle import OracleBatch
    n, seed = 4133, 77
    nw = n_waves(n)
    eng, ora = Batched2048(n, seed=seed), OracleBatch(n, seed)
    rng = np.random.default_rng(seed)
    eng.reset()
    ora.reset()
    for _ in range(40):
        eng.step(None, want_info=False)
        ora.step(None)
    check_slots_match_stats(eng)

    def reset_masked(mask):
        abandoned = _per_slot(np.where((mask != 0) & ~ora.pending, ora.score, 0), n)
        expect, crossing = _plant_gain_edges(eng, ora, -abandoned)
        eng.reset(mask=mask)
        ora.reset(mask=mask)
        assert np.array_equal(eng.get_boards().reshape(n, 16), ora.boards)
        _check_gain(eng, ora, expect, crossing)
        assert ((expect >> np.uint64(32)) == 0)[crossing].all()     # borrowed into high dword 0

    # (a) a masked reset abandons running episodes
    reset_masked(rng.integers(0, 2, n).astype(np.uint8))
    # (b) after steps without auto-reset: a masked reset of pending boards (they stay finished) and running ones
    for _ in range(4):
        eng.step(None, auto_reset=False, want_info=False)
        ora.step(None, auto_reset=False)
    assert np.array_equal(StateBlob(eng).pending(), ora.pending) and ora.pending.sum() > 100
    mask = (ora.pending | (rng.random(n) < 0.5)).astype(np.uint8)
    reset_masked(mask)
    assert np.array_equal(StateBlob(eng).pending(), ora.pending)
    for _ in range(3):                                       # (pending marks again, for the score imports below)
        eng.step(None, auto_reset=False, want_info=False)
        ora.step(None, auto_reset=False)
    assert ora.pending.any()

    # (c) g2048_set_scores lowering and raising, from a host and from a device buffer (pending boards: no delta)
    for where, how in (("host", "lower"), ("device", "raise"), ("device", "lower"), ("host", "raise")):
        old = ora.score.astype(np.int64)
        if how == "lower":
            new = old // 3
        else:
            new = np.minimum(old + 1 + (np.arange(n) * 37) % 5000, (1 << 24) - 1)
        delta = _per_slot(np.where(ora.pending, 0, new - old), n)
        assert ((delta <= 0) if how == "lower" else (delta >= 0)).all()
        expect, crossing = _plant_gain_edges(eng, ora, delta)
        scores = new.astype(np.int32)
        eng.set_scores(torch.as_tensor(scores, device=eng.device) if where == "device" else scores)
        ora.set_scores(scores)
        _check_gain(eng, ora, expect, crossing)
        assert ((expect >> np.uint64(32)) == (0 if how == "lower" else 2))[crossing].all()   # a borrow / a carry

    # (d) g2048_seed on slots whose four high dwords are all non-zero
    blob = StateBlob(eng)
    c = blob.counters()
    s = np.arange(nw, dtype=np.uint64)
    for cnt in (EP, ILL, GAIN, PEND):
        c[:nw, cnt] |= (np.uint64(1) + (s + np.uint64(cnt)) % np.uint64(13)) << np.uint64(32)
    blob.set_counters(c)
    blob.load_into(eng)
    assert (StateBlob(eng).slots[:nw, 4:8] != 0).all()
    eng.seed(seed + 1)
    ora.seed_(seed + 1)
    assert not StateBlob(eng).slots[:nw, 4:8].any()
    fresh = Batched2048(n, seed=seed + 1)
    fresh.set_boards(eng.get_boards())
    fresh.set_scores(eng.get_scores())
    st, want = _readers(eng), _readers(fresh)
    assert st == want and st["episodes"] == 0 and st["return_sum"] == ora.return_sum == 0


# ------------------------------------------------------------------------------------------- readers at full width
SUMMARY_WAVES = 256 * 16      # returns_summary_kernel: kSummaryBlocks blocks of sixteen wavefronts; their grid-stride walk
                              # (kUnroll = 4 waves in flight per trip) gives wavefront g every wave w with w % 4096 == g


def test_readers_at_full_width(torch_cuda):
    """2^26 + a ragged tail of boards with scores near 2^24: a lane of returns_summary_kernel sums 257 live scores
    (> 2^32), a wavefront > 2^38; highest tiles cover every histogram bin; the terminal records' scores add up past 2^32
    and reach 2^24 - 1; the slots' high dwords are non-zero.  Every field of both readers against numpy, three times
    (the summary's arrival counters must be back at zero after each launch)."""
    torch = torch_cuda
    from gym2048_amd.batched import Batched2048, parse_stats
    n = (1 << 26) + 4133
    nw, ns = n_waves(n), n_slots(n)
    rng = np.random.default_rng(26)
    eng = Batched2048(n, seed=5)
    dev = eng.device
    # ---- boards: highest exponent h (every value 0..31), the tile at a varying cell, the other cells h // 2
    h = rng.integers(0, 32, n, dtype=np.uint8)
    h[:32] = np.arange(32)
    ht = torch.as_tensor(h, device=dev)
    cells = (ht // 2).unsqueeze(1).repeat(1, 16)
    cells.scatter_(1, (torch.arange(n, device=dev) % 16).unsqueeze(1), ht.unsqueeze(1))
    eng.set_boards(cells)
    del cells
    scores = ((1 << 24) - 1 - rng.integers(0, 256, n)).astype(np.int32)
    eng.set_scores(torch.as_tensor(scores, device=dev))
    torch.cuda.synchronize()

    blob = StateBlob(eng)
    # ---- terminal records: one tile of exponent 1 (potential 0), so the deficit is -score mod 2^24; every 7th board none
    has = np.arange(n) % 7 != 3
    last = ((1 << 24) - 1 - rng.integers(0, 1 << 20, n)).astype(np.int64)
    last[::1000] = (1 << 24) - 1
    d = (-last) & 0xFFFFFF
    lr = blob.last_records
    lr[:, 0] = has
    for j in range(8):
        lr[:, 8 + j] = np.where(has, ((d >> (3 * j)) & 7) << 5, 0).astype(np.uint8)
    del d
    # ---- slots: non-zero high dwords in every counter; pending marks only where the top lanes do not look
    c = blob.counters()
    s = np.arange(nw, dtype=np.uint64)
    lo = rng.integers(0, M32, (nw, 3), dtype=np.uint64)
    c[:nw, EP] = ((np.uint64(1) + s % np.uint64(255)) << np.uint64(32)) | lo[:, 0]
    c[:nw, ILL] = ((s % np.uint64(17)) << np.uint64(32)) | lo[:, 1]
    c[:nw, GAIN] += ((np.uint64(1) + s % np.uint64(1000)) << np.uint64(32)) | lo[:, 2]
    pend_slot = (np.arange(nw) % SUMMARY_WAVES >= 100) & (np.arange(nw) % 37 == 0) & (np.arange(nw) < nw - 1)
    c[:nw, PEND] = np.where(pend_slot, rng.integers(0, 1 << 63, nw, dtype=np.uint64) | np.uint64(1 << 63), 0)
    c[nw:] = np.uint64((9 << 32) | 0xFFFFFFFF)               # padding slots: never summed
    blob.set_counters(c)
    blob.load_into(eng)
    pending = blob.pending()
    assert pending.sum() > 10_000
    assert np.array_equal(eng.get_last_scores(), np.where(has, last, 0).astype(np.int32))   # the records are what we think
    del blob, lr

    # ---- the reference
    live = np.where(pending, 0, scores).astype(np.int64)
    ep, ill, g = slot_sums(c, n)
    want = dict(episodes=ep, illegal_ends=ill, last_count=int(has.sum()), last_score_sum=int(last[has].sum()),
                last_score_max=(1 << 24) - 1, max_exp=31, highest_hist=np.bincount(h, minlength=32).tolist(),
                return_sum=books_return_sum(g, scores, pending))
    del h, scores, last, has, pending
    assert all(x > 0 for x in want["highest_hist"]) and want["last_score_sum"] > M32
    assert (c[:nw, :3] >> np.uint64(32)).any(axis=0).all()
    # the inputs reach the summary's edge: per-lane `live` of the grid-stride walk (wave w of the batch is walked by
    # wavefront w % SUMMARY_WAVES of the grid), and its 64-lane sum in wave_sum64_lane63
    rounds = -(-nw // SUMMARY_WAVES)
    walk = np.zeros(rounds * SUMMARY_WAVES * 64, np.int64)
    walk[:n] = live
    lane = walk.reshape(rounds, SUMMARY_WAVES, 64).sum(axis=0)
    del walk, live
    assert lane.max() > M32 and lane.sum(axis=1).max() > 1 << 38

    for _ in range(3):
        full = eng.episode_stats()
        dev_full = parse_stats(eng.episode_stats_device())
        summary = parse_stats(eng.episode_stats_device(returns_only=True))
        for st in (full, dev_full):
            for key, v in want.items():
                assert st[key] == v, (key, st[key], v)
        for key in ("episodes", "illegal_ends", "return_sum"):
            assert summary[key] == want[key], (key, summary[key], want[key])
        assert summary["last_score_max"] is None and not any(summary["highest_hist"])
