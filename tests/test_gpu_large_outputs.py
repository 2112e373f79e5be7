"""GPU: outputs of the read-only kernels past 4 GiB (expectimax values, afterstate boards, afterstate observations, the
engine's one-hot observation), where the 64-bit output offsets of g2048_kernels.hip hold values above 2^32.  The pattern of
test_gpu_configs.test_more_than_4_gib_of_records: a periodic batch built on the device (board i = base[i % m]); windows at
the start, across the 4 GiB byte line and at the end equal a small call on the same rows and an independent reference,
and every row equals the reference of its base row.  Each test frees what it allocated before the next one starts."""
import numpy as np
import pytest

from analysis_helpers import assert_rows_periodic, host_search, hs, row_lut, tiled, trajectory_boards  # noqa: F401 (hs, row_lut: fixtures)
from move_lut import lut_afterstates, onehot_ref

pytestmark = pytest.mark.gpu

GIB4 = 1 << 32
WIN = 2048
M = 4099  # odd period: rows one power of two apart are different boards


@pytest.fixture(scope="module")
def g_mod(torch_cuda):
    import gym2048_amd
    return gym2048_amd


@pytest.fixture(scope="module")
def base():
    traj = trajectory_boards()
    b = traj[np.random.default_rng(4).choice(len(traj), M, replace=False)]
    assert len(np.unique(b, axis=0)) == M
    return b


@pytest.fixture
def torch(torch_cuda):
    yield torch_cuda
    torch_cuda.cuda.synchronize()
    torch_cuda.cuda.empty_cache()          # the next test allocates its own 4 GiB+


def windows(n, line_row):
    """Row windows: the first rows, the rows across byte 2^32 of an output of 2^32 / line_row bytes per row, the last."""
    return [(0, WIN), (line_row - WIN // 2, line_row + WIN // 2), (n - WIN, n)]


def test_expectimax_values_past_4_gib(g_mod, torch, hs, base):
    """Depth 1, 2^28 + 4133 boards: 4 GiB + of values (row i at byte 16 i) and of input boards; the kernel strides 64
    times over the grid cap on the way."""
    n = (1 << 28) + 4133
    boards = tiled(torch, base, n)
    s = g_mod.expectimax(boards, 1)
    torch.cuda.synchronize()
    assert s.value.numel() * 4 > GIB4 and boards.numel() > GIB4
    host = host_search(hs, base, 1)
    for a, b in windows(n, GIB4 // 16):
        rows = boards[a:b]
        small = g_mod.expectimax(rows, 1)
        want = host_search(hs, rows.cpu().numpy(), 1)
        assert torch.equal(s.action[a:b], small.action) and torch.equal(s.value[a:b], small.value), a
        assert np.array_equal(s.action[a:b].cpu().numpy(), want[0]) and np.array_equal(s.value[a:b].cpu().numpy(), want[1]), a
    assert_rows_periodic(torch, s.action, torch.as_tensor(host[0]).cuda(), 1 << 24)
    assert_rows_periodic(torch, s.value, torch.as_tensor(host[1]).cuda(), 1 << 24)


def test_afterstate_boards_past_4_gib(g_mod, torch, base, row_lut):
    """2^26 + 4133 boards: 4 GiB + of afterstates (64 B per board, stored as chunk wave_first * 4 + j), with score and legal."""
    n = (1 << 26) + 4133
    boards = tiled(torch, base, n)
    out = g_mod.Afterstates(torch.empty((n, 4, 16), dtype=torch.uint8, device="cuda"),
                            torch.empty((n, 4), dtype=torch.int32, device="cuda"),
                            torch.empty(n, dtype=torch.uint8, device="cuda"), None)
    a = g_mod.afterstates(boards, out=out)
    torch.cuda.synchronize()
    assert a.boards.numel() > GIB4
    new, score, mask = lut_afterstates(base, row_lut)
    for lo, hi in windows(n, GIB4 // 64):
        rows = boards[lo:hi]
        small = g_mod.afterstates(rows)
        want = lut_afterstates(rows.cpu().numpy(), row_lut)
        for k, name in enumerate(("boards", "score", "legal")):
            assert torch.equal(getattr(a, name)[lo:hi], getattr(small, name)), (lo, name)
            assert np.array_equal(getattr(a, name)[lo:hi].cpu().numpy(), want[k]), (lo, name)
    for got, want in zip((a.boards, a.score, a.legal), (new, score, mask)):
        assert_rows_periodic(torch, got, torch.as_tensor(want).cuda(), 1 << 22)


@pytest.mark.parametrize("kind,dtype,n", [("afterstates", "uint8", (1 << 22) + 4133),
                                          ("afterstates", "float32", (1 << 20) + 4133),
                                          ("observe_onehot", "float32", (1 << 22) + 4133)])
def test_observations_past_4_gib(g_mod, torch, base, row_lut, kind, dtype, n):
    """4 GiB + of observations: the afterstates' stack() (4 x 256 / 1 024 B per board, at (wave_first * 4 + 64q) <<
    (4 + dtype)) and the engine's observe_onehot (1 024 B per board in float32, 64-bit chunk index)."""
    dt = getattr(torch, dtype)
    boards = tiled(torch, base, n)
    if kind == "afterstates":
        got = g_mod.afterstates(boards, obs_dtype=dt).obs
        new = torch.as_tensor(lut_afterstates(base, row_lut)[0]).cuda()
        want = onehot_ref(new, dt)                                         # [m, 4, 16, 4, 4]
    else:
        eng = g_mod.Batched2048(n)
        eng.set_boards(boards)
        got = eng.observe_onehot(dt)
        torch.cuda.synchronize()
        eng.close()
        want = onehot_ref(torch.as_tensor(base).cuda(), dt)               # [m, 16, 4, 4]
    torch.cuda.synchronize()
    per_board = got[0].numel() * got.element_size()
    assert got.numel() * got.element_size() > GIB4 and GIB4 % per_board == 0
    for lo, hi in windows(n, GIB4 // per_board):
        rows = boards[lo:hi]
        if kind == "afterstates":
            small = g_mod.afterstates(rows, obs_dtype=dt).obs
            ref_rows = onehot_ref(torch.as_tensor(lut_afterstates(rows.cpu().numpy(), row_lut)[0]).cuda(), dt)
        else:
            e = g_mod.Batched2048(hi - lo)
            e.set_boards(rows)
            small = e.observe_onehot(dt)
            torch.cuda.synchronize()
            e.close()
            ref_rows = onehot_ref(rows, dt)
        assert torch.equal(got[lo:hi], small) and torch.equal(got[lo:hi], ref_rows), lo
    assert_rows_periodic(torch, got, want, 1 << 16)


