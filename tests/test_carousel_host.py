"""CPU: the carousel reference against itself (sequential loop vs numpy twin) and against the g++ build of the header's
carousel functions (tests/host_carousel): stage choice, sample index, ring slot and survival, the seen transition, the
workgroup ranges, and whole steps in the kernels' three passes for several range sizes.  A stand-alone driver of the host
code runs under AddressSanitizer and UBSan."""
import subprocess

import numpy as np
import pytest

import carousel_helpers as ch
import carousel_ref as cref

THR = (8, 16, 32)               # "has an 8", "has a 16", "has a 32" as masks: stage_mask(8) = 1 << 3, ...


@pytest.fixture(scope="module")
def hl():
    return ch.load_host_carousel()


def random_batch(rng, n, p_term=0.25, hi=6):
    # cells below a per-board limit, so that the boards spread over all the stages of THR
    records = (rng.integers(0, 2**16, size=(n, 16)) % rng.integers(1, hi + 1, size=(n, 1))).astype(np.uint8)
    records[:, 8:] |= (rng.integers(0, 8, size=(n, 8)) << 5).astype(np.uint8)      # score bits: carried verbatim
    return records, (rng.random(n) < p_term).astype(np.uint8)


def assert_same(a, b, ra, rb, where):
    assert np.array_equal(ra, rb), f"{where}: records"
    assert np.array_equal(a.pool, b.pool), f"{where}: pool"
    assert a.count == b.count, f"{where}: count {a.count} vs {b.count}"
    assert np.array_equal(a.seen, b.seen), f"{where}: seen"
    assert np.array_equal(a.episodes, b.episodes), f"{where}: episodes"


@pytest.mark.parametrize("n,capacity,thr", [(1, 1, (8,)), (65, 3, THR), (700, 4, THR), (700, 64, (8, 16)), (300, 1, THR)])
def test_sequential_and_vectorised_reference_agree(n, capacity, thr):
    rng = np.random.default_rng(n * 131 + capacity)
    a = cref.Carousel(thr, n, capacity, seed=0x1234567890abcdef)
    b = a.copy()
    trace = {}
    for step in range(10):
        records, term = random_batch(rng, n)
        ra = cref.step(a, records.copy(), term, index_offset=5, trace=trace)
        rb = cref.step_np(b, records.copy(), term, index_offset=5)
        assert_same(a, b, ra, rb, f"step {step}")
    if n >= 65:
        assert all(x > 0 for x in trace["entries"][1:]) and sum(trace["restarts"]) > 0, trace


def test_stage_of_records(hl):
    rng = np.random.default_rng(3)
    records = rng.integers(0, 256, size=(4096, 16)).astype(np.uint8)            # every byte value, spare bits set anywhere
    records[:64, :] &= 0x03
    thr = np.array([0x0008, 0x4000, 0x6000, 0x8000, 0xC000, 0xE000, 0xFFFF], np.uint16)
    out = np.zeros(len(records), np.uint8)
    for S in range(2, 9):
        assert hl.carousel_check_stage(records.ctypes.data, len(records), S, thr.ctypes.data, out.ctypes.data) == 0
        want = np.array([cref.stage(r, thr[:S - 1].tolist()) for r in records], np.uint8)
        assert np.array_equal(out, want), S
        assert np.array_equal(cref.stage_np(records, thr[:S - 1].tolist()), want), S
    assert hl.carousel_check_stage(records.ctypes.data, 1, 1, thr.ctypes.data, out.ctypes.data) == -1
    assert hl.carousel_check_stage(records.ctypes.data, 1, 9, thr.ctypes.data, out.ctypes.data) == -1


def test_stage_choice_and_top(hl):
    rng = np.random.default_rng(4)
    edge = [0, 1, 6, 7, 8, 0x7fffffff, 0x80000000, 0xfffffff8, 0xfffffffe, 0xffffffff]
    cases = [(g, e) for g in edge for e in edge] + [tuple(int(v) for v in rng.integers(0, 2**32, 2)) for _ in range(2000)]
    for top in range(8):
        for g, e in cases:                                    # g + e crosses 2^32 in many of them; e = 0xffffffff included
            assert hl.carousel_check_choice(g, e, top) == cref.stage_choice(g, e, top) == (g + e) % (top + 1)
    for count in ([0, 0], [0, 1], [0, 0, 5, 0], [9, 0, 0, 0], [0, 1, 0, 2**40, 0, 0, 0, 0], [0] * 7 + [1]):
        arr = np.array(count, np.uint64)
        assert hl.carousel_check_top(arr.ctypes.data, len(count)) == cref.top_stage(count)


def test_sample_index(hl):
    rng = np.random.default_rng(5)
    seeds = [0, 1, 0xffffffffffffffff, 0x43524F5500000000, 0x123456789abcdef0]
    for _ in range(3000):
        e, g = (int(v) for v in rng.integers(0, 2**32, 2))
        k, fill, seed = int(rng.integers(1, 8)), int(rng.choice([1, 2, 3, 1000, 65535, 65536])), seeds[int(rng.integers(len(seeds)))]
        j = hl.carousel_check_sample(e, g, k, fill, seed)
        assert j == cref.sample(e, g, k, fill, seed) and 0 <= j < fill
    assert all(hl.carousel_check_sample(e, 7, 3, 1, 99) == 0 for e in (0, 1, 0xffffffff))      # fill = 1
    # the tag separates the stream from the untagged one under an equal seed
    from oracle.cpu_ref import philox4x32_10
    assert cref.sample(1, 2, 3, 65536, 0) != (philox4x32_10((1, 2, 3, 0), (0, 0))[0] * 65536) >> 32


def test_fill_slot_and_survival(hl):
    rng = np.random.default_rng(6)
    counts = [0, 1, 2, 63, 64, 65, 2**32 - 1, 2**32, 2**32 + 12345, 2**40 + 7, 2**64 - 70000]
    for C in (1, 2, 3, 64, 1000, 65535, 65536):
        for count in counts:
            assert hl.carousel_check_fill(count, C) == min(count, C)
            for m in (1, 2, C - 1, C, C + 1, 3 * C + 2, 2**32 - 256):
                if m < 1:
                    continue
                ranks = {0, m - 1, max(m - C, 0), max(m - C - 1, 0), min(m - 1, C), int(rng.integers(0, m))}
                for r in ranks:
                    want = (count + r) % C if r >= m - C else -1
                    assert hl.carousel_check_slot(count, r, m, C) == want, (count, r, m, C)
    # the ring written one entry at a time ends where the rank formula puts the survivors
    for C, count, m in ((1, 5, 4), (3, 2**32 + 1, 7), (64, 100, 200), (64, 10, 3)):
        ring = {}
        for r in range(m):
            ring[(count + r) % C] = r
        by_rank = {hl.carousel_check_slot(count, r, m, C): r for r in range(m) if hl.carousel_check_slot(count, r, m, C) >= 0}
        assert ring == by_rank


def test_seen_transition(hl):
    for seen in list(range(8)) + [0xff]:
        for st in range(8):
            nxt = hl.carousel_check_seen(seen, st)
            if seen == 0xff:
                assert nxt == st and not hl.carousel_check_is_entry(nxt)          # adopts the stage, records nothing
            elif st > seen:
                assert nxt == (st | 0x80) and hl.carousel_check_is_entry(nxt)     # an entry, marked for the scatter pass
            else:
                assert nxt == seen and not hl.carousel_check_is_entry(nxt)
    assert not hl.carousel_check_is_entry(0xff)


def test_ranges(hl):
    for n in (1, 255, 256, 257, 769, 1024 * 256, 1024 * 256 + 1, 2**24 + 77, 2**32 - 256):
        per, groups = cref.ranges(n)
        assert hl.carousel_check_range(n, 256, 1024) == per
        assert per % 256 == 0 and groups <= 1024 and (groups - 1) * per < n <= groups * per


@pytest.mark.parametrize("per", [1, 7, 64, 256, 100000])
def test_whole_steps_in_three_passes(hl, per):
    """The host build's restart / scan / scatter over ranges of any size equals the sequential reference."""
    rng = np.random.default_rng(per)
    for n, C, offset in ((1, 1, 0), (63, 1, 2**32 - 63), (300, 3, 17), (700, 64, 2**31)):
        ref_car = cref.Carousel(THR, n, C, seed=77)
        ref_car.episodes[:] = 0xfffffffe                       # wraps within the run
        host_car = ref_car.copy()
        for step in range(8):
            records, term = random_batch(rng, n)
            want = cref.step(ref_car, records.copy(), term, index_offset=offset)
            got = ch.host_step(hl, host_car, records.copy(), term, index_offset=offset, per=per)
            assert_same(host_car, ref_car, got, want, f"n={n} C={C} step {step}")
        assert n == 1 or (ref_car.episodes < 100).any()        # some board wrapped its episode counter


def test_count_beyond_2_to_32(hl):
    n, C = 200, 3
    rng = np.random.default_rng(9)
    ref_car = cref.Carousel(THR, n, C, seed=1)
    ref_car.count = [0, 2**32 + 1, 2**40 + 2, 0]               # not multiples of C; stage 3 skipped... until entered
    ref_car.pool[:] = rng.integers(0, 256, ref_car.pool.shape)
    host_car = ref_car.copy()
    for step in range(6):
        records, term = random_batch(rng, n)
        want = cref.step(ref_car, records.copy(), term)
        got = ch.host_step(hl, host_car, records.copy(), term, per=64)
        assert_same(host_car, ref_car, got, want, f"step {step}")
    assert ref_car.count[1] > 2**32 + 1


def test_host_code_under_sanitizers():
    """A stand-alone program of the host code (its own main) under -fsanitize=address,undefined."""
    out = subprocess.run([ch.build_sanitized_driver()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "carousel driver ok" in out.stdout and "runtime error" not in out.stderr
