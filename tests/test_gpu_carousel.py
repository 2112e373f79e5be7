"""GPU: carousel shaping (g2048_carousel_step, g2048_carousel_step_plain).  The plain form on crafted
records and the engine form behind real steps equal the reference tests/carousel_ref.py byte for byte -- records, pool,
count, seen and episodes, over successive calls so that state carries -- and the trainers with ``carousel=`` equal the hand
composition of their launches.  Every test shows from the reference or from its input (never from the code under test)
that it reaches the edge it names."""
import numpy as np
import pytest

import carousel_ref as cref
from analysis_helpers import g  # noqa: F401 (fixture)
from carousel_helpers import assert_state_equal, board_with, load_into, record
from ntuple_helpers import TUPLES_17x4

pytestmark = pytest.mark.gpu

THR = (8, 16, 32)                # stage_mask(8), stage_mask(16), stage_mask(32)
STAGE_BOARDS = [board_with(1, 2, 1), board_with(3, 1), board_with(4, 2, 2), board_with(5, 1, 3)]    # a board of stage 0..3
FRESH = record(board_with(0, 0, 0, 0, 0, 1, 0, 0, 0, 2))                                          # what auto-reset leaves: two tiles


def dev(torch, a):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda:0")


def rec_of(stage, i):
    """A record of the given stage whose cells and score bits depend on i, so that no two rows of a test are equal."""
    cells = list(STAGE_BOARDS[stage])
    cells[8 + i % 8] = 1 + (i // 8) % 2
    return record(cells, spare=(i * 2654435761) & 0xffffff)


class Pair:
    """A device Carousel and the reference, stepped together on the plain form."""

    def __init__(self, g, thr, n, capacity, seed=5, offset=0):
        self.dev, self.ref, self.offset = g.Carousel(thr, n, capacity=capacity, seed=seed), cref.Carousel(thr, n, capacity, seed), offset
        self.calls = 0

    def step(self, torch, records, terminated, trace=None, fast=False):
        records = np.ascontiguousarray(records, np.uint8)
        d_rec, d_term = dev(torch, records), dev(torch, np.asarray(terminated, np.uint8))
        self.dev.step_plain(d_rec, d_term, index_offset=self.offset)
        want = (cref.step_np if fast else cref.step)(self.ref, records.copy(), terminated, self.offset, *(() if fast else (trace,)))
        torch.cuda.synchronize()
        assert_state_equal(self.dev, self.ref, d_rec, want, f"call {self.calls}")
        self.calls += 1
        return want


def edge_lanes(n):
    """The first and last lane of every wave, which includes those of every 256-board workgroup range."""
    return sorted({i for w in range(0, n, 64) for i in (w, min(w + 63, n - 1))})


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 3 * 256 + 1])
def test_plain_form_sizes_and_edges(g, torch_cuda, n):
    torch = torch_cuda
    assert cref.ranges(n)[0] == 256 and cref.ranges(3 * 256 + 1) == (256, 4)
    p, trace = Pair(g, THR, n, capacity=3, offset=2**32 - n), {}
    edges = edge_lanes(n)
    zeros = np.zeros(n, np.uint8)
    base = np.array([rec_of(0, i) for i in range(n)])
    p.step(torch, base, zeros, trace)                                          # seen = 0xff adopts stage 0
    assert trace["entries"] == [0, 0, 0, 0] and (p.ref.seen == 0).all()
    recs = base.copy()
    for x, i in enumerate(edges):
        recs[i] = rec_of(1 + x % 3, i)
    p.step(torch, recs, zeros, trace)                                          # entries on the edge lanes
    assert sum(trace["entries"]) == len(edges)
    recs2, term = recs.copy(), zeros.copy()
    for i in edges:
        recs2[i], term[i] = FRESH, 1                                           # the edge lanes end their episodes ...
    for i in range(1, n, 7):
        if not term[i]:
            recs2[i] = rec_of(3, i)                                            # ... while others enter stage 3
    out = p.step(torch, recs2, term, trace)
    if n >= 257:                                                               # (few edge lanes below that: k may be 0 for all)
        assert sum(trace["restarts"]) > 0 and any((out[i] != FRESH).any() for i in edges)
    rng = np.random.default_rng(n)
    for _ in range(3):                                                         # everything at once, state carried along
        recs3 = np.array([rec_of(int(s), i) for i, s in enumerate(rng.integers(0, 4, n))])
        term = (rng.random(n) < 0.3).astype(np.uint8)
        recs3[term != 0] = FRESH
        p.step(torch, recs3, term, trace)
    assert p.ref.episodes.sum() > 0


@pytest.mark.parametrize("capacity", [1, 3, 64])
def test_more_entries_than_capacity(g, torch_cuda, capacity):
    torch = torch_cuda
    n = 3 * 256 + 100
    p = Pair(g, THR, n, capacity)
    zeros = np.zeros(n, np.uint8)
    base = np.array([rec_of(0, i) for i in range(n)])
    p.step(torch, base, zeros)
    enter = sorted(set(edge_lanes(n)) | set(range(5, n, 9)))                   # 100+ entries, every wave and range
    assert len(enter) > 64 + 3
    recs = base.copy()
    for i in enter:
        recs[i] = rec_of(2, i)
    p.step(torch, recs, zeros)
    pool = p.dev.pool.cpu().numpy()
    m = len(enter)
    assert p.ref.count == [0, 0, m, 0] and p.dev.count.cpu().tolist() == [0, 0, m, 0]
    for r in range(m - capacity, m):                                           # the last C by index, each in its slot
        assert np.array_equal(pool[2][r % capacity], recs[enter[r]]), r
    # the same boards end their episodes (and restart from the pool), then enter again: the ring goes on from count mod C
    term = zeros.copy()
    term[enter] = 1
    ended = recs.copy()
    ended[enter] = FRESH
    p.step(torch, ended, term)
    again = enter[: capacity + 2]
    recs = np.array([rec_of(0, i + 1000) for i in range(n)])
    for i in again:
        recs[i] = rec_of(2, i + 2000)
    live = p.ref.seen.copy()
    p.step(torch, recs, zeros)
    made = sum(1 for i in again if live[i] < 2)
    assert made > 0 and p.ref.count[2] == m + made


def test_stage_is_not_monotone_and_unknown_adopts(g, torch_cuda):
    torch = torch_cuda
    thr = (0x4000, 0x6000)
    p, trace = Pair(g, thr, 3, capacity=4), {}
    low, a, b, c = board_with(1, 2), board_with(14, 13, 13), board_with(14, 14), board_with(15)
    assert [cref.stage(record(x), thr) for x in (low, a, b, c)] == [0, 2, 1, 2]
    zeros = np.zeros(3, np.uint8)
    # board 0: low, then 16k+8k+8k -> 16k+16k -> 32k; board 1 starts unknown ON 16k+8k+8k; board 2: low -> 16k+16k -> 32k
    p.step(torch, np.array([record(low), record(low), record(low)]), np.array([0, 1, 0], np.uint8), trace)
    p.dev.seen[1] = 0xff
    p.ref.seen[1] = 0xff
    p.step(torch, np.array([record(a, 1), record(a, 2), record(low)]), zeros, trace)
    assert trace["entries"] == [0, 0, 1] and p.ref.seen.tolist() == [2, 2, 0]       # board 1 adopted its stage: nothing recorded
    p.step(torch, np.array([record(b, 3), record(b, 4), record(b, 5)]), zeros, trace)
    assert trace["entries"] == [0, 1, 1] and p.ref.seen.tolist() == [2, 2, 1]       # only board 2 rose above its seen
    p.step(torch, np.array([record(c, 6), record(c, 7), record(c, 8)]), zeros, trace)
    assert trace["entries"] == [0, 1, 2] and p.ref.seen.tolist() == [2, 2, 2]       # 32k is stage 2 again: new only to board 2
    assert p.ref.count == [0, 1, 2] and np.array_equal(p.dev.pool.cpu().numpy()[2][1], record(c, 8))


def test_pool_is_read_as_of_before_the_call(g, torch_cuda):
    torch = torch_cuda
    n = 130
    p = Pair(g, (8,), n, capacity=2, offset=1)
    base = np.array([rec_of(0, i) for i in range(n)])
    p.step(torch, base, np.zeros(n, np.uint8))
    # board 0 makes the first ever entry into stage 1 while board 129 (g = 130, e = 1 after this call) ends an episode
    recs, term = base.copy(), np.zeros(n, np.uint8)
    recs[0], recs[129], term[129] = rec_of(1, 5), FRESH, 1
    assert cref.stage_choice(130, 0, 1) == 0 and cref.stage_choice(130, 1, 1) == 1
    p.ref.episodes[129] = 1                                                    # so that k would be 1 if the entry were visible
    p.dev.episodes[129] = 1
    out = p.step(torch, recs, term)
    assert np.array_equal(out[129], FRESH) and p.ref.seen[129] == 0 and p.ref.count == [0, 1]
    # one call later the entry is there: the restarted record is the pool's, cells and score bits
    p.ref.episodes[129] = 1
    p.dev.episodes[129] = 1
    out = p.step(torch, recs, term)
    assert np.array_equal(out[129], rec_of(1, 5)) and (out[129] & 0xe0).any() and p.ref.seen[129] == 1


def test_skipped_stage_keeps_the_fresh_board(g, torch_cuda):
    torch = torch_cuda
    n = 64
    p = Pair(g, (8, 16), n, capacity=4, seed=2**64 - 1)
    p.ref.count = [0, 0, 6]                                                    # stage 1 never entered, stage 2 six times
    p.ref.pool[2] = np.array([rec_of(2, 50 + j) for j in range(4)])
    p.ref.seen[:] = 0
    load_into(p.dev, p.ref)
    recs, term = np.array([FRESH] * n), np.ones(n, np.uint8)
    out = p.step(torch, recs, term)
    for i in range(n):
        k = i % 3
        if k == 2:
            assert any(np.array_equal(out[i], q) for q in p.ref.pool[2]) and p.ref.seen[i] == 2
        else:
            assert np.array_equal(out[i], FRESH) and p.ref.seen[i] == 0, (i, k)
    assert len({out[i].tobytes() for i in range(2, n, 3)}) > 1                 # more than one slot was drawn


def test_sparse_entries_in_a_batch_beyond_the_workgroup_cap(g, torch_cuda):
    torch = torch_cuda
    n = 2**24 + 77
    per, groups = cref.ranges(n)
    assert per > 256 and groups < -(-n // 256)                                 # ranges of many chunks
    p = Pair(g, THR, n, capacity=3, seed=9)
    p.ref.count = [0, 2**32 + 2, 2, 0]
    p.ref.pool[1] = np.array([rec_of(1, 70 + j) for j in range(3)])
    p.ref.pool[2][:2] = np.array([rec_of(2, 80 + j) for j in range(2)])
    p.ref.seen[:] = 0
    p.ref.episodes[:] = 0
    p.dev.seen.zero_()
    for name in ("pool", "count"):
        getattr(p.dev, name).copy_(torch.as_tensor({"pool": p.ref.pool, "count": p.ref.count_i64()}[name]))
    recs = np.tile(rec_of(0, 0), (n, 1))
    term = np.zeros(n, np.uint8)
    spots = [0, 63, 64, 255, 256, per - 1, per, per + 1, 7 * per - 1, 7 * per, (groups - 1) * per - 1, (groups - 1) * per, n - 78, n - 1]
    for x, i in enumerate(spots):
        recs[i] = rec_of(1 + x % 3, i)                                         # 14 entries: stage 1 five (> C), 2 five, 3 four
    for i in (1, 65, per + 2, 5 * per + 3, n - 2, 2**24, 2**24 + 1, 2**24 + 2):
        recs[i], term[i] = FRESH, 1
    out = p.step(torch, recs, term, fast=True)
    assert p.ref.count == [0, 2**32 + 7, 7, 4]
    assert sum(1 for i in np.nonzero(term)[0] if (out[i] != FRESH).any()) >= 2
    del out, recs


def test_engine_form_behind_real_steps(g, torch_cuda):
    torch = torch_cuda
    from gym2048_amd.batched import decode_record
    from gym2048_amd.ntuple import stage_mask
    n, steps, offset = 512, 48, 1000
    thr = (stage_mask(8), stage_mask(16), stage_mask(32))
    assert thr == THR
    eng = g.Batched2048(n, seed=11, board_offset=offset)
    try:
        eng.reset()
        car, ref, trace = g.Carousel(thr, n, capacity=16, seed=3), cref.Carousel(thr, n, 16, 3), {}
        for s in range(steps):
            eng.step(None)                                                     # the synthetic random policy, auto-reset on
            before = eng.records().cpu().numpy().copy()
            term = eng.terminated.cpu().numpy()
            car.step(eng)
            want = cref.step(ref, before.copy(), term, index_offset=offset, trace=trace)
            assert_state_equal(car, ref, eng.records(), want, f"step {s}")
            restarted = [i for i in np.nonzero(term)[0] if (want[i] != before[i]).any()]
            if restarted:
                scores = eng.scores().cpu().numpy()
                for i in restarted:
                    assert scores[i] == decode_record(want[i])[1], (s, i)
        # (figures of the reference, not of the kernels: the comparison above is not vacuous)
        assert all(x > 0 for x in trace["entries"][1:]) and all(x > 0 for x in trace["restarts"][1:]), trace
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------ trainers
N_TRAIN, SHIFT, H = 256, 3, 3


def full_boards(n, seed):
    """Full boards of nine tile values: about one in twenty has no move left, and the others few, so episodes end (and
    restart) from the first step on."""
    return np.random.default_rng(seed).integers(1, 10, size=(n, 16)).astype(np.uint8)


class Run:
    """An engine on crowded boards, a staged 17x4 network with random weights, TC accumulators, a trace and a carousel whose
    pool already holds a few boards."""

    def __init__(self, g, torch, seed=7):
        self.g, self.torch = g, torch
        self.eng = g.Batched2048(N_TRAIN, seed=seed)
        self.eng.reset()
        self.eng.set_boards(full_boards(N_TRAIN, seed))
        self.net = g.NTupleNet(TUPLES_17x4, stages=THR)
        gen = torch.Generator(device="cpu").manual_seed(seed)
        self.net.weights.copy_(torch.randint(-(1 << 16), 1 << 16, tuple(self.net.weights.shape), generator=gen, dtype=torch.int32))
        self.tc, self.trace = g.NTupleTC(self.net), g.NTupleTrace(N_TRAIN, depth=H, lam=0.5)
        self.car = g.Carousel(self.net, N_TRAIN, capacity=8, seed=seed)
        ref = cref.Carousel(THR, N_TRAIN, 8, seed)
        ref.count = [0, 3, 9, 2]
        for k in (1, 2, 3):
            ref.pool[k] = np.array([rec_of(k, 10 * k + j) for j in range(8)])
        load_into(self.car, ref)
        self.car.reset()

    def close(self):
        self.eng.close()

    def trainer(self, name, steps, **kw):
        from gym2048_amd import ntuple
        args = {"train": (self.eng, self.net), "tc_train": (self.eng, self.net, self.tc), "tdl_train": (self.eng, self.net, self.trace),
                "tcl_train": (self.eng, self.net, self.tc, self.trace)}[name]
        getattr(ntuple, name)(*args, steps, SHIFT, **kw)

    def by_hand(self, name, steps):
        """The launches of the trainers, written out, with Carousel.step behind the engine's step."""
        net, eng, work = self.net, self.eng, self.g.ntuple.td_work(self.eng)
        for _ in range(steps):
            eng.ntuple_evaluate(net, out=work.before)
            eng.step(work.before.action, auto_reset=True, want_info=False)
            self.car.step(eng)
            eng.ntuple_evaluate(net, out=work.after)
            if name in ("train", "tc_train"):
                work.delta.copy_(work.after.best)
                work.delta.masked_fill_(eng.terminated.bool(), 0)
                work.delta.sub_(work.before.after_value)
            else:
                self.trace.push(work.before.after, work.before.after_value, work.after.best, eng.terminated, work.delta)
            if name == "train":
                net.update(work.before.after, work.delta, SHIFT)
            elif name == "tc_train":
                net.tc_update(work.before.after, work.delta, SHIFT, self.tc)
            elif name == "tdl_train":
                net.trace_update(self.trace, work.delta, SHIFT)
            else:
                net.tc_trace_update(self.trace, work.delta, SHIFT, self.tc)

    def state(self):
        t = self.torch
        t.cuda.synchronize()
        c = self.car
        return [x.clone() for x in (self.net.weights, self.tc.err, self.tc.mag, self.trace.hist, self.trace.len, self.eng.records(),
                                    c.pool, c.count, c.seen, c.episodes)]


def same(torch, a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


TRAINERS = ["train", "tc_train", "tdl_train", "tcl_train"]


@pytest.mark.parametrize("name", TRAINERS)
def test_trainers_with_and_without_a_carousel(g, torch_cuda, name):
    torch, steps = torch_cuda, 10
    import gym2048_amd.ntuple  # noqa: F401 (g.ntuple)
    runs = [Run(g, torch) for _ in range(5)]
    try:
        plain, none, with_car, again, hand = runs
        start = plain.state()
        plain.trainer(name, steps)
        none.trainer(name, steps, carousel=None)
        assert same(torch, plain.state(), none.state())                        # carousel=None: the bits of no keyword at all
        assert not torch.equal(plain.state()[0], start[0])
        with_car.trainer(name, steps, carousel=with_car.car)
        again.trainer(name, steps, carousel=again.car)
        hand.by_hand(name, steps)
        got = with_car.state()
        assert same(torch, got, again.state())                                 # the same seeds: the same bits twice
        assert same(torch, got, hand.state())                                  # the hand composition
        # the carousel did something: episodes ended, boards restarted from the pool, and the run differs from the plain one
        assert int(with_car.car.episodes.sum()) > 0 and not torch.equal(got[5], plain.state()[5])
    finally:
        for r in runs:
            r.close()


def test_state_dict_round_trip_mid_run(g, torch_cuda):
    torch, steps = torch_cuda, 6
    a, b = Run(g, torch), Run(g, torch, seed=8)
    try:
        a.trainer("tcl_train", steps, carousel=a.car)
        saved = (a.eng.state_dict(), a.net.state_dict(), a.tc.state_dict(), a.trace.state_dict(), a.car.state_dict())
        a.trainer("tcl_train", steps, carousel=a.car)
        with pytest.raises(ValueError, match="seed"):
            b.car.load_state_dict(saved[4])
        b.car = g.Carousel(b.net, N_TRAIN, capacity=8, seed=7)
        for obj, state in zip((b.eng, b.net, b.tc, b.trace, b.car), saved):
            obj.load_state_dict(state)
        b.trainer("tcl_train", steps, carousel=b.car)
        assert same(torch, a.state(), b.state())
        assert int(a.car.episodes.sum()) > 0
    finally:
        a.close()
        b.close()
