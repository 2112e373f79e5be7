"""Reference model of carousel shaping (include/g2048.h "Carousel shaping"): the definition as a plain
sequential Python loop over the boards (``step``), and a numpy-vectorised twin for large n (``step_np``) that records the
entries by the rank formula instead of one at a time.  The two are checked against each other (tests/test_carousel_cpu.py);
the host build of the header's functions and the kernels are compared with them.  A plain module, like ntuple_ref."""
import numpy as np

from oracle.cpu_ref import philox4x32_10, philox4x32_10_np

KEY_TAG = 0x43524F55          # "CROU", kCarouselKeyTag
UNKNOWN = 0xff
MASK32 = 0xffffffff


def cell(byte):
    """c(e) of a record byte or a plain exponent: min(byte & 0x1f, 15)."""
    return min(int(byte) & 0x1f, 15)


def stage(rec, thr):
    """stage(b) of a 16-byte record: the number of thresholds the tile mask is not below."""
    m = 0
    for byte in rec:
        m |= 1 << cell(byte)
    return sum(1 for t in thr if m >= t)


def stage_np(records, thr):
    records = np.ascontiguousarray(np.asarray(records, np.uint8).reshape(-1, 16))
    if len(records) > 4096:
        # a large batch is mostly copies of its first row: those rows share its stage, the others are done one by one
        halves = records.view(np.uint64)
        other = np.nonzero((halves[:, 0] != halves[0, 0]) | (halves[:, 1] != halves[0, 1]))[0]
        if len(other) <= len(records) // 64:
            st = np.full(len(records), stage(records[0], thr), np.uint8)
            st[other] = [stage(records[i], thr) for i in other]
            return st
    m = np.zeros(len(records), np.uint32)
    for j in range(16):
        m |= np.uint32(1) << np.minimum(records[:, j] & np.uint8(0x1f), 15).astype(np.uint32)
    st = np.zeros(len(records), np.uint8)
    for t in thr:
        st += (m >= t).astype(np.uint8)
    return st


def top_stage(count):
    return max([k for k in range(1, len(count)) if count[k] > 0], default=0)


def stage_choice(g, e, top):
    return (int(g) + int(e)) % (top + 1)          # Python ints: the sum in as many bits as it needs


def sample(e, g, k, fill, seed):
    w = philox4x32_10((e & MASK32, g & MASK32, k, 0), (seed & MASK32, ((seed >> 32) & MASK32) ^ KEY_TAG))[0]
    return (w * fill) >> 32


class Carousel:
    """The state of a carousel for n boards; ``count`` is a list of Python ints (uint64 on the device)."""

    def __init__(self, thr, n, capacity, seed=0):
        self.thr = tuple(int(t) for t in thr)
        assert 1 <= len(self.thr) <= 7 and all(1 <= t <= 65535 for t in self.thr)
        assert all(a < b for a, b in zip(self.thr, self.thr[1:]))
        assert 1 <= capacity <= 65536
        self.n, self.capacity, self.seed = int(n), int(capacity), int(seed)
        S = len(self.thr) + 1
        self.pool = np.zeros((S, self.capacity, 16), np.uint8)
        self.count = [0] * S
        self.seen = np.full(self.n, UNKNOWN, np.uint8)
        self.episodes = np.zeros(self.n, np.uint32)

    @property
    def n_stages(self):
        return len(self.thr) + 1

    def copy(self):
        c = Carousel(self.thr, self.n, self.capacity, self.seed)
        c.pool, c.count, c.seen, c.episodes = self.pool.copy(), list(self.count), self.seen.copy(), self.episodes.copy()
        return c

    def count_i64(self):
        return np.array(self.count, np.uint64).view(np.int64)


def step(car, records, terminated, index_offset=0, trace=None):
    """The carousel step, one board after the other, in place on ``records`` (uint8 [n, 16]) and ``car``.  ``trace``: a dict
    that receives ``restarts[k]`` and ``entries[k]``, the restarts from and the entries into every stage."""
    records = np.asarray(records)
    assert records.shape == (car.n, 16) and records.dtype == np.uint8
    C = car.capacity
    pool0, count0 = car.pool.copy(), list(car.count)          # as they were before the call
    top = top_stage(count0)
    if trace is not None:
        trace.setdefault("restarts", [0] * car.n_stages)
        trace.setdefault("entries", [0] * car.n_stages)
    for i in range(car.n):
        if terminated[i]:
            e = int(car.episodes[i])
            car.episodes[i] = (e + 1) & MASK32
            g = index_offset + i
            k = stage_choice(g, e, top)
            if k > 0 and count0[k] > 0:
                j = sample(e, g, k, min(count0[k], C), car.seed)
                records[i] = pool0[k][j]
                car.seen[i] = k
                if trace is not None:
                    trace["restarts"][k] += 1
            else:
                car.seen[i] = stage(records[i], car.thr)
        else:
            st = stage(records[i], car.thr)
            if car.seen[i] == UNKNOWN:
                car.seen[i] = st
            elif st > car.seen[i]:
                car.pool[st][car.count[st] % C] = records[i]   # the ring, one entry at a time
                car.count[st] = (car.count[st] + 1) & (2**64 - 1)
                car.seen[i] = st
                if trace is not None:
                    trace["entries"][st] += 1
    return records


def step_np(car, records, terminated, index_offset=0):
    """The same with numpy over the whole batch; the entries by rank: rank r of m into slot (count + r) mod C if r >= m - C."""
    records = np.asarray(records)
    assert records.shape == (car.n, 16) and records.dtype == np.uint8
    C, n = car.capacity, car.n
    term = np.asarray(terminated).astype(bool)
    pool0, count0 = car.pool.copy(), list(car.count)
    top = top_stage(count0)
    st = stage_np(records, car.thr)                             # of the records as they came in
    # restarts
    ti = np.nonzero(term)[0]
    if len(ti):
        e = car.episodes[ti].astype(np.uint64)
        g = ti.astype(np.uint64) + np.uint64(index_offset)
        car.episodes[ti] = ((e + np.uint64(1)) & np.uint64(MASK32)).astype(np.uint32)
        k = ((g + e) % np.uint64(top + 1)).astype(np.int64)    # g + e < 2^33
        made = np.array(count0, dtype=object)[k] if len(k) else k
        use = np.array([kk > 0 and int(mm) > 0 for kk, mm in zip(k, made)], bool)
        new_seen = st[ti].copy()
        if use.any():
            ku, eu, gu = k[use], e[use], g[use]
            fill = np.array([min(count0[kk], C) for kk in ku], np.uint64)
            w = philox4x32_10_np(eu, gu, ku.astype(np.uint64), np.zeros(len(ku), np.uint64), car.seed & MASK32,
                                 ((car.seed >> 32) & MASK32) ^ KEY_TAG)[0].astype(np.uint64)
            j = ((w * fill) >> np.uint64(32)).astype(np.int64)
            records[ti[use]] = pool0[ku, j]
            new_seen[use] = ku.astype(np.uint8)
        car.seen[ti] = new_seen
    # boards that go on
    live = ~term
    unknown = live & (car.seen == UNKNOWN)
    entry = live & ~unknown & (st > car.seen)
    car.seen[unknown] = st[unknown]
    car.seen[entry] = st[entry]
    for k in range(1, car.n_stages):
        idx = np.nonzero(entry & (st == k))[0]                 # ascending board index
        m = len(idx)
        if m == 0:
            continue
        r = np.arange(m)
        keep = r >= m - C
        slots = [(car.count[k] + int(x)) % C for x in r[keep]]
        car.pool[k][slots] = records[idx[keep]]
        car.count[k] = (car.count[k] + m) & (2**64 - 1)
    return records


def ranges(n, block=256, cap=1024):
    """The boards of every workgroup of the carousel kernels (carousel_range of g2048_device.h): (per, groups)."""
    blocks = -(-n // block)
    groups = min(blocks, cap)
    per = -(-blocks // groups) * block
    return per, -(-n // per)
