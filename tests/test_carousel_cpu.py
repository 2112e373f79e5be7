"""CPU: the carousel's public surface without a device -- the package exports it, the three C symbols refuse bad arguments
before any HIP call, and ``Carousel(...)`` checks its arguments, its state and the engine it is given."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge

INVALID = -1      # G2048_ERR_INVALID


@pytest.fixture(scope="module")
def lib():
    ge.build_hip()
    from gym2048_amd import _lib
    return _lib.load()


def test_package_exports_carousel():
    import gym2048_amd
    from gym2048_amd import ntuple
    assert gym2048_amd.Carousel is ntuple.Carousel


class Buffers:
    """Host arrays of the right sizes: a refused call never reads them, and no call here is a valid one."""

    def __init__(self, n=8, S=3, capacity=4):
        self.n = n
        self.records = np.zeros((n + 1, 16), np.uint8)
        self.terminated = np.zeros(n, np.uint8)
        self.pool = np.zeros((S * capacity + 1, 16), np.uint8)
        self.count, self.seen, self.episodes = np.zeros(S, np.uint64), np.zeros(n, np.uint8), np.zeros(n, np.uint32)
        self.scratch = np.zeros(1 << 15, np.uint32)

    def desc(self, S=3, thr=(8, 16), capacity=4, **over):
        from gym2048_amd._lib import CarouselC
        d = CarouselC(S, (C.c_uint16 * 7)(*thr), capacity, 5, self.pool.ctypes.data, self.count.ctypes.data, self.seen.ctypes.data,
                      self.episodes.ctypes.data, self.scratch.ctypes.data)
        for name, value in over.items():
            setattr(d, name, value)
        return d


def refused(lib, rc, *words):
    assert rc == INVALID
    msg = lib.g2048_last_error().decode()
    assert all(w in msg for w in words), msg


def test_scratch_bytes(lib):
    assert lib.g2048_carousel_scratch_bytes(0) == 0
    assert lib.g2048_carousel_scratch_bytes(2**32 - 255) == 0
    small, large = lib.g2048_carousel_scratch_bytes(1), lib.g2048_carousel_scratch_bytes(2**32 - 256)
    assert 0 < small == large <= 1 << 17 and small % 4 == 0            # bounded whatever n is


def test_step_plain_refuses_bad_arguments(lib):
    b = Buffers()
    rec, term, n = b.records.ctypes.data, b.terminated.ctypes.data, b.n

    def call(d, records=rec, n=n, offset=0, terminated=term):
        return lib.g2048_carousel_step_plain(records, n, offset, terminated, None if d is None else C.byref(d), None)

    refused(lib, call(None), "carousel is NULL")
    for S in (0, 1, 9):
        refused(lib, call(b.desc(S=S)), "n_stages")
    refused(lib, call(b.desc(thr=(0, 16))), "thresholds[0]=0")
    refused(lib, call(b.desc(thr=(16, 16))), "strictly ascending")
    refused(lib, call(b.desc(S=4, thr=(8, 16, 9))), "strictly ascending")
    for capacity in (0, 65537):
        refused(lib, call(b.desc(capacity=capacity)), "capacity")
    for field in ("pool", "count", "seen", "episodes", "scratch"):
        refused(lib, call(b.desc(**{field: None})), field, "NULL")
    refused(lib, call(b.desc(), records=None), "records is NULL")
    refused(lib, call(b.desc(), terminated=None), "terminated is NULL")
    refused(lib, call(b.desc(), records=rec + 8), "misaligned")
    refused(lib, call(b.desc(pool=b.pool.ctypes.data + 8)), "misaligned")
    refused(lib, call(b.desc(count=b.count.ctypes.data + 4)), "misaligned")
    refused(lib, call(b.desc(episodes=b.episodes.ctypes.data + 2)), "misaligned")
    for bad_n in (0, 2**32 - 255, 2**40):
        refused(lib, call(b.desc(), n=bad_n), "n=")
    refused(lib, call(b.desc(), offset=2**32 - n + 1), "index_offset")
    refused(lib, call(b.desc(), offset=2**64 - 1), "index_offset")


def test_engine_step_refuses_a_null_engine(lib):
    b = Buffers()
    d = b.desc()
    assert lib.g2048_carousel_step(None, C.byref(d), b.terminated.ctypes.data, None) == INVALID
    assert b"NULL" in lib.g2048_last_error()


def test_carousel_checks_its_arguments(lib):
    from gym2048_amd.ntuple import Carousel, NTupleNet, stage_mask
    with pytest.raises(ValueError, match="staged network"):
        Carousel(NTupleNet("17x4", device="cpu"), 16, device="cpu")
    with pytest.raises(ValueError, match="at least one stage threshold"):
        Carousel((), 16, device="cpu")
    with pytest.raises(ValueError, match="strictly ascending"):
        Carousel((16, 8), 16, device="cpu")
    with pytest.raises(ValueError, match="at most 7"):
        Carousel(range(1, 9), 16, device="cpu")
    for bad in (0, 65537, 2.5):
        with pytest.raises(ValueError, match="capacity"):
            Carousel((8,), 16, capacity=bad, device="cpu")
    for bad in (0, 2**32 - 255):
        with pytest.raises(ValueError, match="n "):
            Carousel((8,), bad, device="cpu")
    with pytest.raises(ValueError, match="seed"):
        Carousel((8,), 16, seed=-1, device="cpu")
    net = NTupleNet("17x4", device="cpu", stages=[stage_mask(16384), stage_mask(16384, 8192)])
    car = Carousel(net, 16, capacity=8, seed=2**64 - 1, device="cpu")
    assert car.stages == (0x4000, 0x6000) and car.n_stages == 3
    assert car.pool.shape == (3, 8, 16) and car.count.shape == (3,) and car.seen.shape == (16,) and car.episodes.shape == (16,)
    assert int(car.seen.min()) == 0xff and car._c.seed == 2**64 - 1 and list(car._c.thresholds)[:2] == [0x4000, 0x6000]


def test_state_dict_round_trip_and_shape_checks(lib):
    import torch
    from gym2048_amd.ntuple import Carousel
    car = Carousel((8, 16), 10, capacity=4, seed=3, device="cpu")
    car.pool.random_(0, 256)
    car.count.copy_(torch.tensor([0, 5, 2**40]))
    car.seen.copy_(torch.tensor([0, 1, 2, 0xff, 0, 1, 2, 0xff, 0, 1], dtype=torch.uint8))
    car.episodes.random_(0, 1000)
    state = car.state_dict()
    other = Carousel((8, 16), 10, capacity=4, seed=3, device="cpu")
    other.load_state_dict(state)
    for name in ("pool", "count", "seen", "episodes"):
        assert torch.equal(getattr(other, name), getattr(car, name)), name
        assert state[name].data_ptr() != getattr(car, name).data_ptr()          # a copy
    other.reset()
    assert int(other.seen.min()) == 0xff and torch.equal(other.pool, car.pool) and torch.equal(other.episodes, car.episodes)
    for key, value in (("stages", (8, 32)), ("capacity", 5), ("seed", 4), ("pool", state["pool"][:, :3]),
                       ("count", state["count"].int()), ("seen", state["seen"][:9]), ("episodes", state["episodes"].long()),
                       ("seen", torch.full((10,), 3, dtype=torch.uint8))):
        with pytest.raises(ValueError):
            other.load_state_dict({**state, key: value})
    with pytest.raises(ValueError, match="Carousel of"):
        from gym2048_amd.ntuple import _carousel_of

        class Engine:
            n_envs, device = 11, torch.device("cpu")
        _carousel_of(Engine(), car)
