"""GPU tests of the small operands of the model-kernel entries (csrc/eofx_abi.hip: fetch_small, stage_small): weights, a trend,
scales, a small matrix and view offsets may lie on the host or on the device.  The engine converts most of them to host
arrays, so the device branch is reached here through the C entries themselves: every case runs once with the operand as a
host array and once as a device tensor, the two outputs must be equal bit for bit, and both must match the float64
restatement of the entry's own test file within that file's bound.
"""

import numpy as np
import pytest

from test_gpu_lowpass import restate as lowpass_restate
from test_gpu_opa import lagged_sum
from test_gpu_orderpos import assert_exact as orderpos_assert_exact
from test_gpu_pcmul import check as pcmul_check
from test_gpu_viewcov import check as viewcov_check

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
N, P = 203, 17            # no multiple of the 64-row tile, the 16-row window or the 16-column block


def either_side(a):
    """(name, operand) pairs: the host array and a device tensor of the same values"""
    import torch

    return [("host", a), ("device", torch.from_numpy(a).cuda())]


def call(ctx, entry, *args):
    from xeofs_amd._lib import ptr, raise_for

    raise_for(getattr(ctx.lib, entry)(ctx.handle, *[ptr(a) if isinstance(a, np.ndarray) or hasattr(a, "data_ptr") else a for a in args]),
              ctx.handle)


@pytest.mark.parametrize("ntau", [3, 66], ids=["fused", "written"])
def test_lagcov_weights(ctx, ntau):
    import torch

    rng = np.random.default_rng(ntau)
    S = rng.standard_normal((N, P)).astype(np.float32)
    Sd = torch.from_numpy(S).cuda()
    w = rng.standard_normal(ntau) * rng.choice([1e-3, 1.0, 10.0], ntau)
    ref, bound = lagged_sum(S, w)
    got = {}
    for side, wx in either_side(w):
        M = torch.empty((P, P), dtype=torch.float64, device="cuda")
        call(ctx, "eofx_lagcov_f64", Sd, N, P, Sd.stride(0), wx, ntau, M)
        got[side] = M.cpu().numpy()
        assert np.all(np.abs(got[side] - ref) <= 2.0 * (N + ntau + 2) * U53 * bound), side
    assert np.array_equal(got["host"], got["device"])


def test_lowpass_weights_and_trend(ctx):
    import torch

    from xeofs_amd.single.lfca import linear_trend

    h = 5
    rng = np.random.default_rng(5)
    S = (rng.standard_normal((N, P)) + 0.02 * rng.standard_normal(P) * np.arange(N)[:, None]).astype(np.float32)
    Sd = torch.from_numpy(S).cuda()
    w = rng.standard_normal(h + 1) * rng.choice([1e-3, 1.0, 10.0], h + 1)
    trend = np.ascontiguousarray(linear_trend(S) * (1.0 + 0.3 * rng.standard_normal((2, P))))
    Yref, Rref, Ybar, B = lowpass_restate(S, w, trend)
    got = {}
    for wside, wx in either_side(w):
        for tside, tx in either_side(trend):
            R = torch.empty((P, P), dtype=torch.float64, device="cuda")
            Y = torch.empty((N, P), dtype=torch.float64, device="cuda")
            call(ctx, "eofx_lowpass_cov_f64", Sd, N, P, Sd.stride(0), wx, h, tx, R, Y)
            R, Y = R.cpu().numpy(), Y.cpu().numpy()
            assert np.all(np.abs(R - Rref) <= 2.0 * (N + 2 * (2 * h + 4)) * U53 * B), (wside, tside)
            assert np.all(np.abs(Y - Yref) <= 2.0 * (2 * h + 4) * U53 * Ybar), (wside, tside)
            got[wside, tside] = (R, Y)
    R0, Y0 = got["host", "host"]
    for key, (R, Y) in got.items():
        assert np.array_equal(R, R0) and np.array_equal(Y, Y0), key


def test_orderpos_scale(ctx):
    import torch

    p, n = 5, 37
    rng = np.random.default_rng(37)
    T = rng.standard_normal((p, n)).astype(np.float32)
    T[1, ::3] = T[1, 0]                                                          # ties
    Td = torch.from_numpy(T).cuda()
    scale = rng.random(p) * 2.7 + 1.0 / 3.0
    got = {}
    for side, sx in either_side(scale):
        q = torch.empty((p, n), dtype=torch.int32, device="cuda")
        z = torch.empty((p, n), dtype=torch.float32, device="cuda")
        call(ctx, "eofx_orderpos_f32", Td, p, n, n, sx, q, n, z, n)
        orderpos_assert_exact(q, z, T, scale)
        got[side] = (q.cpu().numpy(), z.cpu().numpy())
    assert np.array_equal(got["host"][0], got["device"][0])
    assert np.array_equal(got["host"][1].view(np.uint32), got["device"][1].view(np.uint32))


def test_pcmul_matrix(ctx):
    import torch

    rows, a, b = 33, 7, 5
    rng = np.random.default_rng(33)
    X = (rng.standard_normal((rows, a)) * rng.choice([1e-3, 1.0, 30.0], (1, a))).astype(np.float32)
    M = rng.standard_normal((a, b)) * rng.choice([1e-2, 1.0, 10.0], (a, 1))
    Xd = torch.from_numpy(X).cuda()
    got = {}
    for side, mx in either_side(M):
        Y = torch.empty((rows, b), dtype=torch.float64, device="cuda")
        call(ctx, "eofx_pcmul_f64", Xd, 0, rows, a, a, mx, b, Y, 1, b)            # EOFX_PCMUL_F32 in, EOFX_PCMUL_F64 out
        got[side] = Y.cpu().numpy()                                              # (a device M returns without a synchronisation)
        pcmul_check(ctx, X, M, got[side], np.float64, f"small operand: M on the {side}")
    assert np.array_equal(got["host"], got["device"])


def test_viewcov_offsets(ctx):
    import torch

    off = np.array([0, 5, 17], dtype=np.int32)
    rng = np.random.default_rng(17)
    Z = (rng.standard_normal((N, P)) * rng.choice([1e-3, 1.0, 30.0], (1, P)) + rng.standard_normal((1, P))).astype(np.float32)
    Zd = torch.from_numpy(Z).cuda()
    mean = torch.sum(Zd, dim=0, dtype=torch.float64).div_(N).contiguous()
    got = {}
    for side, ox in either_side(off):
        Cm = torch.empty((P, P), dtype=torch.float64, device="cuda")
        call(ctx, "eofx_viewcov_f64", Zd, N, P, Zd.stride(0), mean, ox, 2, 0, Cm, P)
        got[side] = Cm.cpu().numpy()
        viewcov_check(got[side], Z, off.tolist(), True, False, f"small operand: off on the {side}")
    assert np.array_equal(got["host"], got["device"])
