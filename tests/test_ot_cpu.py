"""The OT matching rule (ot_ref.py, include/clipfs.h "OT matching") and the plan's closed forms without a GPU: the
marginals of the plan hold, the degenerate shapes have their closed forms, the detached gradient is scale * T, fp32
stays finite at the eps bound, and clipfs_ot_plan is the arithmetic the header states."""
import pytest
import torch

import ot_ref as R

CASES = tuple(R.CASES)


@pytest.mark.parametrize("feat", ("spread", "concentrated"))
@pytest.mark.parametrize("marg", ("uniform", "random"))
def test_marginals_hold_after_100_iterations(feat, marg):
    X, P, mu, nu = R.inputs("plot", feat, marg)
    out = R.forward(X, P, mu, nu, eps=0.1, iters=100)
    B, M, C, N, _ = R.CASES["plot"]
    mu, nu = R.marginals(B, M, C, N, mu, nu, torch.float64)
    T = out["T"]
    assert float((T.sum(3) - mu[:, None, :]).abs().max()) <= 1e-8
    assert float((T.sum(2) - nu[None, :, :]).abs().max()) <= 1e-8
    assert float((T.sum((2, 3)) - nu.sum(1)[None, :]).abs().max()) <= 1e-8  # 1 up to the fp32 rounding of nu


@pytest.mark.parametrize("iters", (1, 5))
def test_one_prompt_gives_the_row_marginal(iters):
    X, P, mu, nu = R.inputs("two_rows_n1", "spread", "random")
    out = R.forward(X, P, mu, nu, eps=0.1, iters=iters, scale=7.0)
    T, z = out["T"], out["z"]
    mu = mu.double() / mu.double().sum(1, keepdim=True)  # the fp32-rounded rows sum to 1 within 2^-24 only; nu is 1
    assert float((T[..., 0] - mu[:, None, :]).abs().max()) <= 1e-15
    want = 7.0 * (mu[:, None, :] * z[..., 0]).sum(2)
    assert float((out["logits"] - want).abs().max()) <= 1e-13


def test_one_row_gives_the_column_marginal():
    X, P, mu, nu = R.inputs("one_row", "spread", "random")
    out = R.forward(X, P, mu, nu, eps=0.1, iters=3)
    assert float((out["T"][:, :, 0, :] - nu.double()[None]).abs().max()) <= 1e-15


def test_detached_gradient_is_scale_times_the_plan():
    """Central differences of scale * sum(T z) in X and P with T held at its value: the function is linear in z, so the
    difference quotient is exact up to rounding."""
    X, P, mu, nu = R.inputs((2, 5, 3, 4, 8), "spread", "random")
    scale, eps, iters = 3.0, 0.2, 20
    dl = torch.randn(2, 3, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    _, dP, dX = R.grads(X, P, dl, mu, nu, eps, iters, scale)
    T = R.forward(X, P, mu, nu, eps, iters, scale)["T"]
    G = dl[:, :, None, None] * scale * T
    assert torch.allclose(dP, torch.einsum("bcmn,bmd->cnd", G, X.double()), rtol=0, atol=1e-13)
    assert torch.allclose(dX, torch.einsum("bcmn,cnd->bmd", G, P.double()), rtol=0, atol=1e-13)

    def f(Xd, Pd):
        return float((dl * scale * (T * torch.einsum("bmd,cnd->bcmn", Xd, Pd)).sum((2, 3))).sum())

    h = 1e-4
    g = torch.Generator().manual_seed(2)
    for _ in range(4):
        dXd, dPd = torch.randn(X.shape, generator=g, dtype=torch.float64), torch.randn(P.shape, generator=g, dtype=torch.float64)
        fd = (f(X.double() + h * dXd, P.double()) - f(X.double() - h * dXd, P.double())) / (2 * h)
        assert abs(fd - float((dX * dXd).sum())) <= 1e-9 * (1 + abs(fd))
        fd = (f(X.double(), P.double() + h * dPd) - f(X.double(), P.double() - h * dPd)) / (2 * h)
        assert abs(fd - float((dP * dPd).sum())) <= 1e-9 * (1 + abs(fd))


@pytest.mark.parametrize("case", CASES)
def test_fp32_stays_finite_at_the_eps_bound(case):
    """eps = 0.05 with z = -1 present: K = exp(-40), and u, v, T stay finite in fp32 for 1, 100 and 1000 iterations."""
    X, P, mu, nu = R.inputs(case, "concentrated", "random")
    for iters in (1, 100, 1000):
        out = R.forward(X, P, mu, nu, eps=0.05, iters=iters, dtype=torch.float32)
        assert float(out["z"].min()) <= -1 + 1e-6 and float(out["z"].max()) >= 1 - 1e-6
        for k in ("u", "v", "T", "logits"):
            assert bool(torch.isfinite(out[k]).all()), (case, iters, k)


@pytest.mark.parametrize("case", CASES)
def test_plan_closed_forms(case):
    from clipfs import _lib, ops
    B, M, C, N, d = R.CASES[case]
    p = ops.ot_plan(B, M, C, N, d)
    assert p == _lib.ot_plan(B, M, C, N, d)
    assert (p["fwd_launches"], p["dp_launches"], p["dx_launches"], p["threads"]) == (1, 1, 1, 256)
    rt, rpl = -(-M // 32), -(-M // 64)
    assert p["rows_per_lane"] == (rpl if rpl <= 2 else 4)
    assert p["prompt_regs"] == next(k for k in (4, 8, 16, 32) if N <= k)
    chunk = min(C, max(1, (128 if rt <= 3 else 64) // N))
    assert p["class_chunk"] == chunk and p["class_chunks"] == -(-C // chunk)
    assert p["z_stride"] == 32 * (-(-chunk * N // 32)) + 1
    assert p["fwd_grid"] == B * p["class_chunks"]
    assert p["fwd_lds_bytes"] == 4 * 32 * rt * p["z_stride"] <= 160 * 1024
    for side, own in (("dp", C * N), ("dx", B * M)):
        gx = -(-own // 32)
        feat = 512 if gx * (-(-d // 512)) >= 256 else 128
        assert (p[side + "_grid_x"], p[side + "_feat_chunk"], p[side + "_grid_y"]) == (gx, feat, -(-d // feat))
    assert p["bwd_lds_bytes"] == 4 * (2 * 32 * 132 + 4 * 32 * 33 + 32 * 32 + 128) <= 64 * 1024


def test_plan_of_the_largest_forward_workgroup():
    from clipfs import ops
    p = ops.ot_plan(1, 256, 2, 32, 4)
    assert p["fwd_lds_bytes"] == 66560 > 64 * 1024  # the forward asks the runtime for it
    assert ops.ot_plan(256, 49, 403, 4, 512)["fwd_grid"] == 256 * 13
