"""The OT matching rule of include/clipfs.h ("OT matching") in torch on the CPU, parameterised by dtype: the reference of
test_ot_cpu.py, test_ot_gpu.py and test_plot_gpu.py.  Inputs are fp32 tensors (so fp32-rounded), evaluated in fp64 (the
reference) or in fp32 (the yardstick of what fp32 costs).  Nothing here imports the package.

    inputs(case, feat, marg, seed)   X [B, M, d], P [C, N, d] unit rows, mu, nu (or None), with z = -1 and z = +1 cells
    forward(...)                     logits, T, z, u, v
    grads(...)                       dP, dX by autograd with T detached
"""
import torch

EPS32 = 2.0 ** -24
# B, M, C, N, d: each the smallest shape that reaches a distinct code path of the kernels
CASES = {
    "plot": (3, 49, 5, 4, 64),          # PLOT's geometry
    "two_rows_n1": (2, 70, 3, 1, 32),   # two rows per lane; N = 1
    "one_row": (2, 1, 3, 4, 36),        # one row; d not a multiple of 32
    "four_rows": (2, 196, 4, 8, 64),    # four rows per lane
    "n_cap": (2, 50, 3, 32, 64),        # N at its cap
    "straddle": (1, 33, 70, 5, 128),    # N does not divide 32: classes straddle column tiles, several class chunks
    "caps": (1, 256, 2, 32, 4),         # both caps; smallest d
}


def unit(x):
    return x / x.norm(dim=-1, keepdim=True)


def inputs(case, feat="spread", marg="uniform", seed=0):
    """fp32 (X, P, mu, nu) for a case name or a (B, M, C, N, d) tuple.  feat: "spread" (random unit rows) or
    "concentrated" (random + 3 x a common direction: z in 0.8 .. 0.95, like real CLIP features).  marg: "uniform" (None,
    None) or "random" (0.5 + rand, normalised).  The first row of P is -X[0, 0] and the last +X[0, 0]: z = -1 and z = +1."""
    B, M, C, N, d = CASES[case] if isinstance(case, str) else case
    g = torch.Generator().manual_seed(1234 + seed)
    X = torch.randn(B, M, d, generator=g, dtype=torch.float64)
    P = torch.randn(C, N, d, generator=g, dtype=torch.float64)
    if feat == "concentrated":
        common = unit(torch.randn(d, generator=g, dtype=torch.float64)) * d ** 0.5
        X, P = X + 3.0 * common, P + 3.0 * common
    else:
        assert feat == "spread", feat
    X, P = unit(X).float(), unit(P).float()
    P.view(C * N, d)[0] = -X[0, 0]
    P.view(C * N, d)[-1] = X[0, 0]
    mu = nu = None
    if marg == "random":
        mu = 0.5 + torch.rand(B, M, generator=g, dtype=torch.float64)
        nu = 0.5 + torch.rand(C, N, generator=g, dtype=torch.float64)
        mu, nu = (mu / mu.sum(1, keepdim=True)).float(), (nu / nu.sum(1, keepdim=True)).float()
    else:
        assert marg == "uniform", marg
    return X, P, mu, nu


def marginals(B, M, C, N, mu, nu, dtype):
    mu = torch.full((B, M), 1.0 / M, dtype=dtype) if mu is None else mu.to(dtype)
    nu = torch.full((C, N), 1.0 / N, dtype=dtype) if nu is None else nu.to(dtype)
    return mu, nu


def sinkhorn(z, mu, nu, eps, iters):
    """(T, u, v) for z [B, C, M, N]: v = 1, then `iters` times u = mu / (K v), v = nu / (K^T u)."""
    K = torch.exp((z - 1.0) / eps)
    B, C, M, N = z.shape
    v = torch.ones(B, C, N, dtype=z.dtype)
    u = None
    for _ in range(iters):
        u = mu[:, None, :] / (K * v[:, :, None, :]).sum(3)
        v = nu[None, :, :] / (K * u[:, :, :, None]).sum(2)
    return u[:, :, :, None] * K * v[:, :, None, :], u, v


def forward(X, P, mu=None, nu=None, eps=0.1, iters=100, scale=100.0, dtype=torch.float64):
    """dict(logits [B, C], T, z [B, C, M, N], u [B, C, M], v [B, C, N]) evaluated in ``dtype``."""
    X, P = X.to(dtype), P.to(dtype)
    B, M, _ = X.shape
    C, N, _ = P.shape
    mu, nu = marginals(B, M, C, N, mu, nu, dtype)
    z = torch.einsum("bmd,cnd->bcmn", X, P)
    with torch.no_grad():
        T, u, v = sinkhorn(z.detach(), mu, nu, eps, iters)
    return dict(logits=scale * (T * z).sum((2, 3)), T=T, z=z, u=u, v=v)


def grads(X, P, dlogits, mu=None, nu=None, eps=0.1, iters=100, scale=100.0, dtype=torch.float64):
    """(logits, dP, dX) in ``dtype``: autograd of sum(dlogits * logits) with T detached."""
    X = X.to(dtype).clone().requires_grad_(True)
    P = P.to(dtype).clone().requires_grad_(True)
    out = forward(X, P, mu, nu, eps, iters, scale, dtype)
    (out["logits"] * dlogits.to(dtype)).sum().backward()
    return out["logits"].detach(), P.grad, X.grad


def tolerance(ref64, ref32, factor=16.0):
    """factor x max(the error of the fp32 evaluation against the fp64 one, 2^-24 max |ref|): nothing from the device."""
    e32 = float((ref32.double() - ref64).abs().max())
    return factor * max(e32, EPS32 * float(ref64.abs().max())), e32
