"""GPU: every selectable instantiation of ntuple_play_log_kernel<T, Shape> and ntuple_log_delta_kernel<T, Shape>
(g2048_ntuple_play_log, g2048_ntuple_log_delta) -- NtupleShape and NtupleStagedShape (S = 3) at T = 1..8,
NtupleMixedShape (S = 3) at T = 2..8, as test_gpu_ntuple_td.py enumerates them: 23 of the 24 compiled of each; the mixed shape
at T = 1 cannot be selected (a network of one list is never mixed).  n = 65, M = 2, full-range random weights: one play_log
against the composition ntuple_evaluate -> step on a twin engine, slot by slot, and one log_delta per slot against
NTupleNet.values on the slot views plus integer arithmetic.  The input guard -- all three flag values and an ended entry below
slot M -- is taken from the composition on the twin engine, which is existing code, not from the pure-Python reference: a play
trace of the reference for each of the 23 networks would be most of this module's run time; tests/test_gpu_ntuple_log.py takes
its guards from the reference."""
import pytest

from ntuple_log_helpers import assert_device_logs_equal, assert_engines_equal, close, composed_play_log, engine, family_case, net_of, values_delta

pytestmark = pytest.mark.gpu
FAMILY_CASES = [(f, T) for f in ("uniform", "staged") for T in range(1, 9)] + [("mixed", T) for T in range(2, 9)]
N, M = 65, 2


@pytest.fixture(scope="module")
def g(torch_cuda):
    import gym2048_amd
    return gym2048_amd


@pytest.mark.parametrize("family, T", FAMILY_CASES, ids=[f"{f}-{T}" for f, T in FAMILY_CASES])
def test_every_instantiation(g, torch_cuda, family, T):
    torch = torch_cuda
    net = net_of(g, torch, family_case(family, T))
    assert net.n_tuples == T and (net.mixed, net.n_stages) == {"uniform": (False, 1), "staged": (False, 3), "mixed": (True, 3)}[family]
    a, b = engine(g, N), engine(g, N)
    log, want = g.NTupleLog(N, depth=M), g.NTupleLog(N, depth=M)
    composed_play_log(b, net, want)
    assert set(want.flag[1:].unique().tolist()) == {0, 1, 3} and bool((want.flag[1] & 2).any()), "inputs: every flag value, an end below slot M"
    a.ntuple_play_log(net, log)
    assert_device_logs_equal(log, want, f"{family} T={T}")
    assert_engines_equal(a, b, f"{family} T={T}")
    nonzero = 0
    for m in range(M):
        expect = values_delta(net, log, m, log.flag)
        got = net.log_delta(log, m)
        assert torch.equal(got, expect), f"{family} T={T} slot {m}: boards {torch.nonzero(got != expect)[:8, 0].tolist()}"
        nonzero += int((expect != 0).sum())
    assert nonzero >= 30
    close(a, b)
