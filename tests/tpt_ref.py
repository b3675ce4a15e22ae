"""fp64 reference of the test-time prompt tuning objective (clipfs_tpt_objective) and the inputs its tests share.

Plain random unit vectors at a logit scale of 100 saturate the confident views (entropy ~1e-9, loss ~log K, a gradient of
~1e-5 that is ill-conditioned): ``tpt_inputs`` draws class features around a common mean and views that lean towards
one class by a varying amount, which gives entropies between ~0.005 and ~6.6 and gradients of order 0.02 - 3."""
import torch


def _unit(t):
    return t / t.norm(dim=-1, keepdim=True)


def tpt_inputs(V, C, d, seed):
    """(F [V, d], T [C, d]) fp32 unit rows; one generator per seed, this draw order."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    m = _unit(r(d))
    R = _unit(r(C, d))
    T = _unit(m + 0.5 * R)
    cls = torch.randint(C, (V,), generator=g)
    a = torch.linspace(0.05, 0.45, V, dtype=torch.float64)[torch.randperm(V, generator=g)]
    N = _unit(r(V, d))
    F = _unit(m + 0.5 * (a[:, None] * R[cls] + (1 - a * a).sqrt()[:, None] * N))
    return F.float(), T.float()


def tpt_ref(F, T, K, s, selected=None, dtype=torch.float64):
    """loss, dT [C, d], H [V], selected [K] (int64, ascending) in fp64 with autograd.  The selection is the K views of
    lowest entropy by a stable sort (ties to the lower index), or ``selected`` when given.  ``dtype=torch.float32``: the
    same expressions evaluated in fp32, the yardstick of the range tests."""
    F = F.detach().to(dtype).cpu()
    T = T.detach().to(dtype).cpu().clone().requires_grad_()
    lp = torch.log_softmax(s * F @ T.t(), dim=-1)
    H = -(lp.exp() * lp).sum(-1)
    if selected is None:
        selected = torch.sort(H.detach(), stable=True).indices[:K]
    sel = torch.sort(selected.detach().cpu().long()).values
    assert sel.numel() == K
    pbar = lp[sel].exp().sum(0) / K
    loss = -(pbar * pbar.log()).sum()
    loss.backward()
    return loss.detach(), T.grad.detach(), H.detach(), sel


def tpt_closed_form(F, T, sel, s):
    """dT of the objective by its closed form: dz_v = (1/K) p_v (g - <p_v, g>), g = -log pbar; dT = s sum dz_v^T F_v."""
    F, T = F.double().cpu(), T.double().cpu()
    K = sel.numel()
    p = torch.softmax(s * F[sel] @ T.t(), dim=-1)
    g = -(p.sum(0) / K).log()
    dz = p * (g[None, :] - (p * g[None, :]).sum(-1, keepdim=True)) / K
    return s * dz.t() @ F[sel]


def entropy_gap(H, K):
    """H_(K+1) - H_(K) of the sorted entropies (inf when K == V)."""
    hs = torch.sort(H).values
    return float("inf") if K >= hs.numel() else (hs[K] - hs[K - 1]).item()
