"""Engineered late-game boards for the step kernels (numpy only: no GPU, no torch).

Random play from reset() reaches tiles of about 2^8, a score deficit of a few dozen and a board with one empty cell only
by accident.  The families here START where the per-board code of g2048_device.h can be wrong: the spawn into the last
empty cell and the end test behind it, full boards that move only by merging, terminal boards (the illegal-move reset
draws other Philox words), max_tile, the "+4" carry through the whole 24-bit deficit field, and 2^16 / 2^17 merges.

Every family is a pure function of a seed.  It carries its boards (uint8 [n, 16] exponents 0..17), scores, first actions
and the configuration it is played under, and a `check` that takes the ORACLE's state after the family's first step and
asserts that the family reached what it names -- conditions on the inputs, proven on the CPU by tests/test_late_game_host.py.
The spawn stream is keyed by the global board index, so a family is always played at its own `offset`: what the CPU test
proves about the oracle's spawns then holds for the same boards on the GPU.
"""
import numpy as np

UP, RIGHT, DOWN, LEFT = 0, 1, 2, 3                       # game2048_env.py:196
SCORE_LIMIT = 1 << 24                                    # scores are exact below it (g2048_device.h)
SEED = 2048                                              # the seed the tests use: every family's check holds for it
BANDS = (1, 3, 10)                                       # checkerboard value bands, each 8 wide (the last one ends at 2^17)
_BLACK = (np.arange(16) // 4 + np.arange(16) % 4) % 2 == 0
# the 24 adjacent cell pairs: 12 in rows (merged by left / right), 12 in columns (merged by up / down)
PAIRS = [(4 * r + c, 4 * r + c + 1) for r in range(4) for c in range(3)] + [(4 * r + c, 4 * r + c + 4) for r in range(3) for c in range(4)]
_PAIR_DIRS = [(LEFT, RIGHT)] * 12 + [(UP, DOWN)] * 12


# ------------------------------------------------------------------------------------------------ plain numpy board facts
def potential(boards):
    """sum over the tiles of (e - 1) * 2^e, int64 [n] (the record's deficit is potential - score mod 2^24)."""
    e = np.asarray(boards).astype(np.int64).reshape(-1, 16)
    return np.where(e > 0, (e - 1) << e, 0).sum(axis=1)


def legal_moves(boards):
    """bool [n, 4]: does direction d change the board?  A line moves when a tile has an empty cell in front of it or two
    equal tiles touch (equal tiles behind a gap are covered by the first rule)."""
    g = np.asarray(boards).reshape(-1, 4, 4)
    out = np.zeros((len(g), 4), bool)
    for d, v in ((LEFT, g), (RIGHT, g[:, :, ::-1]), (UP, g.transpose(0, 2, 1)), (DOWN, g.transpose(0, 2, 1)[:, :, ::-1])):
        front, back = v[:, :, :-1], v[:, :, 1:]
        out[:, d] = (((front == 0) & (back != 0)) | ((front == back) & (front != 0))).any(axis=(1, 2))
    return out


def equal_pairs(boards):
    """number of adjacent pairs of equal tiles, int [n]"""
    g = np.asarray(boards).reshape(-1, 4, 4)
    rows = (g[:, :, :-1] == g[:, :, 1:]) & (g[:, :, :-1] != 0)
    cols = (g[:, :-1] == g[:, 1:]) & (g[:, :-1] != 0)
    return rows.sum(axis=(1, 2)) + cols.sum(axis=(1, 2))


def after_boards(o):
    """The board every episode stands on after the step's move and spawn, whether or not it was reset afterwards."""
    done = o.terminated.astype(bool)
    return np.where(done[:, None], o.terminal_boards, o.boards)


def spawned(before, o):
    """(four, two): bool [n], the value the step spawned; both False where the move was illegal.  A merge raises the
    potential by what it scores, a spawned 2 leaves it alone, a spawned 4 adds 4."""
    legal = o.illegal == 0
    grew = potential(after_boards(o)) - potential(before) - np.where(legal, o.reward, 0).astype(np.int64)
    assert np.isin(grew[legal], (0, 4)).all() and (grew[~legal] == 0).all()
    return legal & (grew == 4), legal & (grew == 0)


def check_scores(o):
    """Every score the oracle holds stays in the range the record keeps exactly."""
    for s in (o.score, o.last_score):
        assert (s >= 0).all() and (s < SCORE_LIMIT).all()


def record_deficit(records):
    """d of raw engine records uint8 [n, 16]: bit k sits in bit 5 + k % 3 of byte 8 + k // 3 (include/g2048.h)."""
    raw = np.asarray(records).astype(np.int64)
    return sum(((raw[:, 8 + k // 3] >> (5 + k % 3)) & 1) << k for k in range(24))


def install(batch, fam):
    """The family's boards, scores, clock and configuration into an OracleBatch-shaped object (in numpy-RNG mode: after
    its seed_numpy)."""
    batch.illegal_move_reward, batch.max_exp = fam.illegal_move_reward, fam.max_exp
    batch.boards[:] = fam.boards
    batch.set_scores(fam.scores)
    batch.t, batch.fresh = fam.clock, False
    return batch


class Family:
    def __init__(self, name, boards, scores, actions, check, max_tile=None, illegal_move_reward=-3.5, clock=(1 << 32) + 1000,
                 offset=0):
        self.name = name
        self.boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 16)
        self.scores = np.ascontiguousarray(scores, dtype=np.int32)
        self.actions = None if actions is None else np.ascontiguousarray(actions, dtype=np.uint8)
        self._check, self.max_tile, self.illegal_move_reward, self.clock, self.offset = check, max_tile, illegal_move_reward, clock, offset
        assert self.boards.max() <= 17 and self.scores.shape == (self.n,) and (self.scores >= 0).all()
        assert (self.scores < SCORE_LIMIT).all() and (self.actions is None or self.actions.shape == (self.n,))

    @property
    def n(self):
        return len(self.boards)

    @property
    def max_exp(self):
        return int(self.max_tile).bit_length() - 1 if self.max_tile else 0

    def check(self, o):
        """o: the oracle (or anything with its fields) after this family's first step from the engineered state."""
        check_scores(o)
        self._check(self, o)


def _scores(rng, n):
    return rng.integers(0, 1 << 20, n)


def _rng(seed, salt):
    return np.random.default_rng([seed, salt])


def checkerboard(rng, n, base):
    """Full boards without equal neighbours: odd exponents on the black cells, even ones on the white, in base .. base+7."""
    k = 2 * rng.integers(0, 4, (n, 16))
    return np.where(_BLACK, base + (base + 1) % 2 + k, base + base % 2 + k).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- rows
def rows_boards():
    """All 18^4 rows of exponents 0..17, four rows per board, in the orientations left / up / right / down."""
    rows = np.array(np.meshgrid(*[np.arange(18)] * 4, indexing="ij")).reshape(4, -1).T.astype(np.uint8)
    g = rows.reshape(-1, 4, 4)
    return {LEFT: g, UP: g.transpose(0, 2, 1), RIGHT: g[:, :, ::-1], DOWN: g.transpose(0, 2, 1)[:, ::-1, :]}


def rows_family(seed=SEED):
    by_dir = rows_boards()
    order = (LEFT, UP, RIGHT, DOWN)
    per = len(by_dir[LEFT])
    boards = np.concatenate([np.ascontiguousarray(by_dir[d]).reshape(per, 16) for d in order])
    actions = np.repeat(np.array(order, np.uint8), per)

    def check(f, o):
        g = f.boards.reshape(4, per, 4, 4)
        back = (g[0], g[1].transpose(0, 2, 1), g[2][:, :, ::-1], g[3][:, ::-1, :].transpose(0, 2, 1))
        for lines in back:                                   # every orientation holds every row exactly once
            codes = (lines.reshape(-1, 4).astype(np.int64) * 18 ** np.arange(4)[::-1]).sum(axis=1)
            assert np.array_equal(np.sort(codes), np.arange(18 ** 4))
        ill = o.illegal.reshape(4, per).astype(bool)
        assert ill.any(axis=1).all() and (~ill).any(axis=1).all()
        assert np.array_equal(~ill.reshape(-1), legal_moves(f.boards)[np.arange(f.n), f.actions])

    return Family("rows", boards, (np.arange(len(boards)) * 7919) % (1 << 20), actions, check, illegal_move_reward=-1.0, clock=7,
                  offset=3 << 20)


# ------------------------------------------------------------------------------------------------------------ one hole
def one_hole_family(seed=SEED, per_band=4096):
    rng = _rng(seed, 1)
    i = np.arange(per_band * len(BANDS))
    boards = np.concatenate([checkerboard(rng, per_band, b) for b in BANDS])
    boards[i, i % 16] = 0
    actions = (i // 16) % 4

    def check(f, o):
        hole, act = np.arange(f.n) % 16, f.actions
        legal, ended = o.illegal == 0, o.terminated != 0
        four, two = spawned(f.boards, o)
        assert legal.sum() == f.n * 3 // 4                   # a tile slides into the hole unless the hole is at the far edge
        pair = hole * 4 + act
        assert len(np.unique(pair[legal])) == 48
        for p in np.unique(pair[legal]):                     # the end test decides both ways behind every (hole, direction)
            assert (ended & legal & (pair == p)).any() and (~ended & legal & (pair == p)).any(), p
        assert (~ended[~legal]).sum() == 0                   # (an illegal move ends the episode)
        assert (four & ended).any() and (four & ~ended).any() and (two & ended).any() and (two & ~ended).any()
        slid = legal & (o.reward == 0)                       # (the tiles on both sides of the hole may be equal and merge)
        assert (after_boards(o) != 0).all(axis=1)[slid].all() and slid.sum() > legal.sum() // 2   # the spawn took the last empty cell

    return Family("one_hole", boards, _scores(rng, len(boards)), actions, check)


# ---------------------------------------------------------------------------------------------------------------- full
def full_a_family(seed=SEED, per_band=256):
    rng = _rng(seed, 2)
    boards = np.concatenate([checkerboard(rng, per_band, b) for b in BANDS])

    def check(f, o):
        assert not legal_moves(f.boards).any()               # illegal in all four directions
        assert (o.illegal == 1).all() and (o.terminated == 1).all() and (o.reward == np.float32(f.illegal_move_reward)).all()
        assert np.array_equal(after_boards(o), f.boards)     # nothing moved, nothing spawned

    return Family("full_a", boards, _scores(rng, len(boards)), np.arange(len(boards)) % 4, check)


def one_pair_boards(rng, n, bases):
    """Full boards with exactly ONE pair of equal neighbours: board j has it at PAIRS[j % 24], value band bases[(j // 48) % len]."""
    j = np.arange(n)
    boards = np.zeros((n, 16), np.uint8)
    bad = np.ones(n, bool)
    p = np.array(PAIRS)[j % 24]
    while bad.any():
        for k, b in enumerate(bases):
            sel = bad & ((j // 48) % len(bases) == k)
            boards[sel] = checkerboard(rng, int(sel.sum()), b)
        boards[j, p[:, 1]] = boards[j, p[:, 0]]
        bad = equal_pairs(boards) != 1
    return boards


def one_pair_actions(n):
    j = np.arange(n)
    return np.array(_PAIR_DIRS)[j % 24, (j // 24) % 2]


def _pair_index(boards):
    g = boards.reshape(-1, 16)
    which = np.full(len(g), -1)
    for k, (a, b) in enumerate(PAIRS):
        which[g[:, a] == g[:, b]] = k
    return which


def full_b_family(seed=SEED, reps=16):
    rng = _rng(seed, 3)
    n = 24 * 2 * len(BANDS) * reps
    boards = one_pair_boards(rng, n, BANDS)

    def check(f, o):
        assert (f.boards != 0).all() and (equal_pairs(f.boards) == 1).all()
        which = _pair_index(f.boards)
        ended = o.terminated != 0
        for k in range(24):                                  # every pair, merged from both of its directions
            for d in _PAIR_DIRS[k]:
                assert ((which == k) & (f.actions == d)).any(), (k, d)
        assert (legal_moves(f.boards).sum(axis=1) == 2).all() and (o.illegal == 0).all()
        e = f.boards[np.arange(f.n), np.array(PAIRS)[which, 0]].astype(np.int64)
        assert np.array_equal(o.reward, (2 << e).astype(np.float32))
        assert (after_boards(o) != 0).all()                  # the spawn filled the only hole
        assert ended.any() and (~ended).any()

    return Family("full_b", boards, _scores(rng, n), one_pair_actions(n), check)


# ------------------------------------------------------------------------------------------------------------ max tile
def _legal_action(boards, turn):
    """A legal direction of every board (the turn[i]-th of its legal ones); every board must have one."""
    legal = legal_moves(boards)
    count = legal.sum(axis=1)
    assert (count > 0).all()
    rank = np.cumsum(legal, axis=1) - 1
    return np.argmax(legal & (rank == (turn % count)[:, None]), axis=1)


def _sparse(rng, n, lo, hi, min_empty=0, max_empty=15):
    """Boards of exponents lo..hi with min_empty..max_empty empty cells at random places."""
    b = rng.integers(lo, hi + 1, (n, 16))
    empties = min_empty + np.arange(n) % (max_empty - min_empty + 1)
    order = rng.permuted(np.tile(np.arange(16), (n, 1)), axis=1)
    b[order < empties[:, None]] = 0
    return b.astype(np.uint8)


CREATE, HOLD, LARGER, FULL = 0, 1, 2, 3


def max_tile_family(seed=SEED, per_kind=256):
    """max_tile = 2048: boards whose move creates the tile (with and without empty cells left), boards that hold it and
    move legally, boards that hold only larger tiles (highest != max_tile: no end), and full boards."""
    rng = _rng(seed, 4)
    n, j = per_kind, np.arange(per_kind)
    p = np.array(PAIRS)[j % 24]
    create = _sparse(rng, n, 1, 9, 0, 14)                    # tiles below 2^10, every fill level up to full ...
    create[j, p[:, 0]] = create[j, p[:, 1]] = 10             # ... and one pair of 2^10 that the action merges
    hold = _sparse(rng, n, 1, 9, 1, 14)
    hold[j, (hold != 0).argmax(axis=1)] = 11
    larger = _sparse(rng, n, 12, 17, 1, 15)
    full = np.concatenate([checkerboard(rng, n // 4, 3), checkerboard(rng, n // 4, 4), one_pair_boards(rng, n // 2, (3, 2))])
    boards = np.concatenate([create, hold, larger, full])
    actions = np.concatenate([one_pair_actions(n), _legal_action(hold, j), _legal_action(larger, j),
                              j[: n // 4] % 4, j[: n // 4] % 4, one_pair_actions(n // 2)])
    kind = np.repeat([CREATE, HOLD, LARGER, FULL], n)

    def check(f, o):
        legal, ended = o.illegal == 0, o.terminated != 0
        after = after_boards(o)
        left = (after == 0).sum(axis=1)
        before_top = f.boards.max(axis=1)
        c, h, lg, fu = (kind == k for k in (CREATE, HOLD, LARGER, FULL))
        assert (before_top[c] == 10).all() and legal[c].all() and (o.highest[c] == 11).all() and ended[c].all()
        assert (c & (left > 0)).any() and (c & (left == 0)).any()          # ends with empty cells left, and without
        assert (before_top[h] == 11).all() and legal[h].all() and ended[h].all() and (left[h] > 0).any()
        assert (np.where(f.boards[lg] == 0, 99, f.boards[lg]).min(axis=1) > 11).all() and legal[lg].all()
        assert (~ended[lg]).sum() > per_kind // 2 and (left[lg & ended] == 0).all()   # only a full board ends there
        assert (f.boards[fu] != 0).all() and (~legal[fu]).any() and (fu & legal & (o.highest == 11)).any()
        assert (f.boards[fu] == 11).any() and ended[fu & ~legal].all()

    return Family("max_tile_2048", boards, _scores(rng, len(boards)), actions, check, max_tile=2048, illegal_move_reward=0.5,
                  clock=(1 << 33) + 5)


def max_tile_top_family(seed=SEED, n=256):
    """The largest max_tile the engine accepts, 2^31: no board of the input domain reaches it, so nothing may end by it."""
    rng = _rng(seed, 5)
    high = _sparse(rng, n, 12, 17, 0, 14)
    high[np.arange(n), (np.arange(n) * 4) % 16] = high[np.arange(n), (np.arange(n) * 4) % 16 + 1] = 17
    full = np.concatenate([checkerboard(rng, n // 2, 10), one_pair_boards(rng, n // 2, (10,))])
    boards = np.concatenate([high, full])
    actions = np.concatenate([np.where(np.arange(n) % 2, LEFT, RIGHT), np.arange(n // 2) % 4, one_pair_actions(n // 2)])

    def check(f, o):
        legal, ended = o.illegal == 0, o.terminated != 0
        full_after = (after_boards(o) != 0).all(axis=1)
        assert (~ended | ~legal | full_after).all() and (legal & ~ended).any() and (legal & ended).any() and (~legal).any()
        assert (o.highest == 18).any()

    return Family("max_tile_top", boards, _scores(rng, len(boards)), actions, check, max_tile=1 << 31, illegal_move_reward=0.5,
                  clock=(1 << 33) + 5)


# --------------------------------------------------------------------------------------------------------------- carry
CARRY_DEFICITS = [(1 << k) - 4 for k in range(3, 25)] + [0x555554, 0xAAAAAC, 0x2AAAA8, 0x955554]
WAVE = 64


def carry_family(seed=SEED):
    """Half-empty boards of tiles <= 2^6 whose action is legal and cannot end the game (eight empty cells), with the
    score set so that the record's deficit d = (potential - score) mod 2^24 is 2^k - 4 for k = 3..24 -- a spawned 4 then
    carries through k - 2 deficit bits and the cell bits between them, from register r[2] into r[3] for k > 12, and wraps to 0
    at k = 24 -- plus alternating-bit values.  Every d sits on 64 consecutive boards, one wavefront.

    The score must stay in [0, 2^24) while the board is played on.  d <= potential: score = potential - d >= 0 and small;
    the tiles are drawn from lo..6 with 8 * (lo - 1) * 2^lo >= d.  Larger d (from 4092): score = 2^24 + potential - d; tiles
    2 and 4 only, so that potential <= 32 and whatever twelve steps can add (the tiles sum to at most 32 + 12 * 4 = 80, a board
    of that sum scores less than 80 * 6) stays far below d - potential >= 4060."""
    rng = _rng(seed, 6)
    boards, scores = [], []
    for d in CARRY_DEFICITS:
        if d <= 2044:
            lo = next(e for e in range(1, 7) if 8 * (e - 1) * (1 << e) >= d)
            b = rng.integers(lo, 7, (WAVE, 16))
        else:
            b = rng.integers(1, 3, (WAVE, 16))
        order = rng.permuted(np.tile(np.arange(16), (WAVE, 1)), axis=1)
        b[order < 8] = 0
        boards.append(b)
        scores.append((potential(b) - d) % SCORE_LIMIT)
    boards, scores = np.concatenate(boards).astype(np.uint8), np.concatenate(scores)
    want_d = np.repeat(CARRY_DEFICITS, WAVE)

    def check(f, o):
        assert np.array_equal((potential(f.boards) - f.scores) % SCORE_LIMIT, want_d)
        assert ((f.boards == 0).sum(axis=1) == 8).all() and f.boards.max() <= 6
        assert (o.illegal == 0).all() and (o.terminated == 0).all()
        four, two = spawned(f.boards, o)
        for g in range(len(CARRY_DEFICITS)):
            s = slice(g * WAVE, (g + 1) * WAVE)
            assert four[s].any() and two[s].any(), hex(CARRY_DEFICITS[g])

    return Family("carry", boards, scores, _legal_action(boards, np.arange(len(boards))), check)


# ---------------------------------------------------------------------------------------------------------------- high
def high_family(seed=SEED, n=2048):
    """Exponents 12..17 at every fill level 1..16; boards 0, 1 mod 4 carry a pair of 2^17 / 2^16 tiles that the action merges
    (alone on the board at fill levels 1 and 2: the reward then is exactly the one merge)."""
    rng = _rng(seed, 7)
    i = np.arange(n)
    fill = 1 + (i // 4) % 16
    b = rng.integers(12, 18, (n, 16))
    order = rng.permuted(np.tile(np.arange(16), (n, 1)), axis=1)
    b[order >= fill[:, None]] = 0
    planted = i % 4 < 2
    pair = np.array(PAIRS)[(i // 4) % 24]
    only = planted & (fill <= 2)
    b[only] = 0
    b[i[planted], pair[planted, 0]] = b[i[planted], pair[planted, 1]] = np.where(i % 4 == 0, 17, 16)[planted]
    actions = np.where(planted, np.array(_PAIR_DIRS)[(i // 4) % 24, (i // 96) % 2], i % 4)

    def check(f, o):
        assert f.boards[f.boards != 0].min() >= 12
        assert np.array_equal(np.unique((f.boards != 0).sum(axis=1)), np.arange(1, 17))
        assert (o.illegal[planted] == 0).all()
        assert (o.reward == np.float32(1 << 18)).any() and (o.reward == np.float32(1 << 17)).any()
        assert (o.reward[only] == np.where(i % 4 == 0, 1 << 18, 1 << 17)[only]).all()
        assert (after_boards(o) == 18).any() and (o.highest == 18).any()
        assert (o.terminated != 0).any() and (o.illegal != 0).any()

    return Family("high", b.astype(np.uint8), _scores(rng, n), actions, check)


# ----------------------------------------------------------------------------------------------------------- the batch
BASE_OFFSET = 1 << 20


def mixed_families(seed=SEED, total=20480):
    """Every family that plays under the common configuration (all but rows and the max-tile ones), at consecutive offsets:
    their concatenation is one batch of `total` boards, a whole number of 256-lane blocks."""
    fams = [one_hole_family(seed), full_a_family(seed), full_b_family(seed), carry_family(seed)]
    rest = total - sum(f.n for f in fams)
    assert rest >= 1024 and total % 256 == 0
    fams.append(high_family(seed, rest))
    off = BASE_OFFSET
    for f in fams:
        f.offset = off
        off += f.n
    return fams


def concat(fams, drop=0):
    """One family-shaped batch of several families at consecutive offsets (without its last `drop` boards)."""
    first = fams[0]
    for a, b in zip(fams, fams[1:]):
        assert b.offset == a.offset + a.n
        assert (b.max_tile, b.illegal_move_reward, b.clock) == (first.max_tile, first.illegal_move_reward, first.clock)
    n = sum(f.n for f in fams) - drop
    spans, start = [], 0
    for f in fams:
        spans.append((f, start, min(start + f.n, n)))
        start += f.n

    def check(f, o):
        for fam, a, b in spans:
            if b - a == fam.n:                               # (a family that lost boards to `drop` is not judged)
                fam.check(_Rows(o, a, b))

    return Family("+".join(f.name for f in fams), np.concatenate([f.boards for f in fams])[:n],
                  np.concatenate([f.scores for f in fams])[:n], np.concatenate([f.actions for f in fams])[:n], check,
                  first.max_tile, first.illegal_move_reward, first.clock, first.offset)


class _Rows:
    """Rows a..b of an oracle's per-board fields."""

    def __init__(self, o, a, b):
        for name in ("boards", "score", "reward", "terminated", "illegal", "highest", "terminal_boards", "last_score"):
            setattr(self, name, getattr(o, name)[a:b])


def max_tile_families(seed=SEED):
    a, b = max_tile_family(seed), max_tile_top_family(seed)
    a.offset = BASE_OFFSET + (1 << 16)
    b.offset = a.offset + a.n
    return [a, b]


def all_families(seed=SEED):
    return [rows_family(seed)] + mixed_families(seed) + max_tile_families(seed)
