"""Shared by the n-tuple move-log tests (g2048_ntuple_play_log, g2048_ntuple_log_delta, g2048_ntuple_log_sweep,
g2048_ntuple_log_train): the host build of the device header's play_log step and delta rule in the kernels'
lane structure (tests/host_ntuple_log, g++) behind ctypes, and what the tests assert from the reference alone before they
compare anything.  A plain module, like ntuple_td_helpers, whose boards and networks it reuses."""
import ctypes as C
import types

import numpy as np

import late_game as lg
import ntuple_log_ref as lref
from host_build import Desc, build_host
from ntuple_play_helpers import ENGINEERED_CLOCK

K_BLOCK = 256


class HostLog(C.Structure):
    """struct HostLog of log_check.cpp."""
    _fields_ = [("depth", C.c_uint32), ("after", C.c_void_p), ("gain", C.c_void_p), ("flag", C.c_void_p)]


def build_host_log(force=False):
    """g++ build of tests/host_ntuple_log (the device header's play_log step and delta rule compiled for the host; tests only)."""
    return build_host("host_ntuple_log", "log_check.cpp", "liblog_check.so", force)


def load_host_log():
    lib = C.CDLL(build_host_log())
    P, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    lib.log_check_play.restype = C.c_int64
    lib.log_check_play.argtypes = [P, u64, u64, u64, u64, u32, C.POINTER(Desc), P, C.POINTER(HostLog), P, P]
    lib.log_check_delta.restype = C.c_int64
    lib.log_check_delta.argtypes = [u64, C.POINTER(Desc), P, C.POINTER(HostLog), u32, P, P]
    return lib


def host_log_of(log):
    """(HostLog over the arrays of an ntuple_log_ref.Log, which must stay alive and contiguous)."""
    for a in (log.after, log.gain, log.flag):
        assert a.flags["C_CONTIGUOUS"]
    return HostLog(log.depth, log.after.ctypes.data, log.gain.ctypes.data, log.flag.ctypes.data)


def host_play_rounds(lib, case, records, M, rounds, max_exp=0):
    """``rounds`` consecutive play_log calls of the host build from ``records`` (not modified) at late_game.BASE_OFFSET, the first
    move at transaction ENGINEERED_CLOCK + 1: the log after each call, the records after the last, the terminal records, the
    counts and what every call returned."""
    rec = np.ascontiguousarray(records, np.uint8).copy()
    n = len(rec)
    log = lref.Log(n, M)
    out = types.SimpleNamespace(logs=[], lanes=[], last_records=np.zeros((n, 16), np.uint8))
    counts = np.zeros(3, np.uint64)
    for r in range(rounds):
        h = host_log_of(log)
        out.lanes.append(lib.log_check_play(rec.ctypes.data, n, lg.SEED, ENGINEERED_CLOCK + 1 + r * M, lg.BASE_OFFSET, max_exp, C.byref(case.desc),
                                            case.w32.ctypes.data, C.byref(h), out.last_records.ctypes.data, counts.ctypes.data))
        out.logs.append(log.copy())
    out.records = rec
    out.episodes, out.illegal_ends, out.gain_sum = (int(c) for c in counts)
    return out


def host_delta(lib, case, log, m, flag=None):
    """(delta int64 [n], ntuple_value calls made, lanes) of the host build for slot m; ``flag``: other flag bytes."""
    work = log.copy()
    if flag is not None:
        work.flag = np.ascontiguousarray(flag, np.uint8)
    delta, evals = np.full(log.n, 0x5a5a5a5a5a5a5a5a, np.int64), np.zeros(1, np.uint64)
    h = host_log_of(work)
    lanes = lib.log_check_delta(log.n, C.byref(case.desc), case.w32.ctypes.data, C.byref(h), m, delta.ctypes.data, evals.ctypes.data)
    return delta, int(evals[0]), lanes


def all_flag_bytes(M, n, seed=11):
    """Random flag bytes [M+1, n] that hold every value 0..255 (where (M + 1) * n >= 256: the first 256 entries count up)."""
    flag = np.random.default_rng(seed).integers(0, 256, size=(M + 1, n)).astype(np.uint8)
    k = min(256, flag.size)
    flag.reshape(-1)[:k] = np.arange(k, dtype=np.uint8)
    return flag


def one_stage_case():
    """"17x4" with the weights of ntuple_td_helpers.uniform_case as a one-stage ntuple_staged_ref.StagedNet: the form the batch-mean
    reference is written for; the unstaged network on the device and in the host build."""
    import ntuple_staged_ref as sref
    from ntuple_play_helpers import cached
    from ntuple_td_helpers import uniform_case

    def make():
        u = uniform_case()
        rnet = sref.StagedNet(u.tuples, (), u.rnet.frac_bits, u.rnet.weights.copy()[None])
        return types.SimpleNamespace(name="17x4-S1", rnet=rnet, w32=u.w32, tuples=u.tuples, stages=None, desc=u.desc)
    return cached("log one-stage case", make)


def assert_log_case(logs, n, M):
    """From the reference alone: the run of n boards over two rounds of M moves is what the tests are there for."""
    r = lref.reaches(logs)
    assert r.empty_slot0, "first round: slot 0 is empty"
    assert len(logs) < 2 or r.carried_slot0, "second round: slot 0 carries slot M"
    if n == 1:
        assert logs[0].flag[1, 0] == 0                                  # its only board has no legal move at the first move
        return r
    assert len(logs) < 2 or r.carried_live, "second round: slot 0 carries entries that were played"
    assert r.values == {0, lref.VALID, lref.VALID | lref.ENDED}, r.values
    if M > 1:
        assert r.ended_below_M and r.ended_with_valid_successor
    return r


# ------------------------------------------------------------------------------------------------ the device side (GPU tests)
SENTINEL = 0xA5


def net_of(g, torch, case):
    """A fresh NTupleNet of a case (ntuple_td_helpers.CASES, or a family case below) with its weights on the device."""
    net = g.NTupleNet(case.tuples, frac_bits=case.rnet.frac_bits, stages=case.stages, mixed=True)
    net.weights.copy_(torch.from_numpy(np.ascontiguousarray(case.w32)).reshape(net.weights.shape))
    return net


_family_cases = {}


def family_case(family, T):
    """Network T of a family of ntuple_deep_helpers (uniform, staged, mixed; full-range random int32) as a case for net_of."""
    from ntuple_deep_helpers import family_net, w32_of
    if (family, T) not in _family_cases:
        rnet = family_net(family, T)
        _family_cases[family, T] = types.SimpleNamespace(name=f"{family}-{T}", rnet=rnet, w32=w32_of(rnet).reshape(-1), tuples=tuple(rnet.tuples),
                                                         stages=getattr(rnet, "thr", None))
    return _family_cases[family, T]


def engine(g, n, board_offset=lg.BASE_OFFSET, first=0, **kw):
    """An engine of n boards holding boards first .. first + n - 1 of ntuple_td_helpers.start_of at ENGINEERED_CLOCK, seed
    late_game.SEED: at first = 0 and BASE_OFFSET the engine ntuple_td_helpers.reference_steps describes."""
    from ntuple_td_helpers import start_of
    eng = g.Batched2048(n, seed=lg.SEED, board_offset=board_offset + first, **kw)
    boards, scores = start_of(first + n)
    eng.set_boards(boards[first:])
    eng.set_scores(scores[first:].astype(np.int32))
    eng.set_clock(ENGINEERED_CLOCK)
    return eng


def close(*engines):
    for e in engines:
        e.close()


def state(eng):
    keeps = eng.last_records_enabled
    return types.SimpleNamespace(records=eng.records().clone(), clock=eng.clock, stats=eng.episode_stats(),
                                 last=eng.last_records().clone() if keeps else None, scores=eng.last_scores().clone() if keeps else None)


def assert_engines_equal(a, b, where):
    import torch
    sa, sb = state(a), state(b)
    assert torch.equal(sa.records, sb.records), f"{where}: records differ on boards {torch.nonzero((sa.records != sb.records).any(1))[:8, 0].tolist()}"
    assert sa.clock == sb.clock, f"{where}: clock {sa.clock} vs {sb.clock}"
    assert sa.stats == sb.stats, f"{where}: episode_stats {sa.stats} vs {sb.stats}"
    assert (sa.last is None) == (sb.last is None)
    if sa.last is not None:
        assert torch.equal(sa.last, sb.last), f"{where}: last_records"
        assert torch.equal(sa.scores, sb.scores), f"{where}: last_scores"


def assert_engines_equal_and_stay_equal(a, b, where):
    assert_engines_equal(a, b, where)
    for _ in range(20):
        a.step(None)
        b.step(None)
    assert_engines_equal(a, b, where + ", 20 steps later")


def composed_play_log(eng, net, want):
    """One play_log call made of existing calls: the carry on ``want`` (an NTupleLog used as plain tensors), then M rounds of
    ntuple_evaluate -> step(action, auto-reset) on ``eng``, each round's outputs written into its slot."""
    import torch
    from gym2048_amd import ntuple
    M = want.depth
    for t in (want.after, want.gain, want.flag):
        t[0].copy_(t[M])
    for m in range(1, M + 1):
        ev = eng.ntuple_evaluate(net)
        legal = (ev.value != ntuple.ILLEGAL).any(dim=1)
        eng.step(ev.action, auto_reset=True, want_info=False)
        want.after[m].copy_(ev.after)
        want.gain[m].copy_(ev.best - ev.after_value)
        ended = torch.where(eng.terminated.bool(), ntuple.LOG_ENDED, 0)
        want.flag[m].copy_(torch.where(legal, ntuple.LOG_VALID | ended, 0).to(torch.uint8))


def assert_device_logs_equal(got, want, where):
    import torch
    for name in ("flag", "gain", "after"):
        a, b = getattr(got, name), getattr(want, name)
        if not isinstance(b, torch.Tensor):
            b = torch.from_numpy(np.ascontiguousarray(b)).to(a.device)
        assert a.shape == b.shape, f"{where}: {name} shape"
        for m in range(a.shape[0]):
            assert torch.equal(a[m], b[m]), f"{where}: {name} of slot {m} differs on boards " \
                                            f"{torch.nonzero((a[m] != b[m]).reshape(a.shape[1], -1).any(1))[:8, 0].tolist()}"


def guarded_log(g, torch, n, M, guard_slots=1):
    """An NTupleLog whose three tensors are the front of larger buffers: (log, guards), guards = the bytes behind slot M of each
    (``guard_slots`` more slots), filled with SENTINEL."""
    log = g.NTupleLog(n, depth=M)
    guards = {}
    for name, width, dtype, shape in (("after", 16, torch.uint8, (M + 1, n, 16)), ("gain", 8, torch.int64, (M + 1, n)),
                                      ("flag", 1, torch.uint8, (M + 1, n))):
        used = (M + 1) * n * width
        raw = torch.full((used + guard_slots * n * width,), SENTINEL, dtype=torch.uint8, device=log.device)
        raw[:used].zero_()
        setattr(log, name, raw[:used].view(dtype).reshape(shape))
        guards[name] = raw[used:]
    from gym2048_amd import _lib
    log._c = _lib.NTupleLogC(M, log.after.data_ptr(), log.gain.data_ptr(), log.flag.data_ptr())
    return log, guards


def load_log(torch, log, rlog):
    """Copy an ntuple_log_ref.Log into a device NTupleLog of the same shape."""
    for name in ("after", "gain", "flag"):
        getattr(log, name).copy_(torch.from_numpy(np.ascontiguousarray(getattr(rlog, name))))
    return log


def values_delta(net, log, m, flag):
    """log_delta(m) from NTupleNet.values on the slot views plus integer arithmetic (torch int64 wraps); ``flag``: the uint8
    [M+1, n] flag bytes to read."""
    import torch
    f, f1 = flag[m].to(torch.int64), flag[m + 1].to(torch.int64)
    v0, v1 = net.values(log.slot(m)), net.values(log.slot(m + 1))
    zero = torch.zeros_like(v0)
    full = log.gain[m + 1] + v1 - v0
    out = torch.where((f1 & 1) != 0, full, zero)
    out = torch.where((f & 2) != 0, -v0, out)
    return torch.where((f & 1) != 0, out, zero)
