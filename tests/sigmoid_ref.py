"""fp64 reference of the pairwise sigmoid (SigLIP) objective (clipfs_sigmoid_objective, include/clipfs.h).  The inputs
and the shapes are those of the InfoNCE tests (contrastive_ref.contrastive_inputs, contrastive_ref.CASES), imported and
not copied.  Three regimes of (t, b): SigLIP's initial point (10, -10), where every cell is saturated and the loss is a
sum of R N softplus tails; (100, -10), mixed; (1, 0), every cell in the linear region."""
import functools
import math

import torch

from contrastive_ref import CASES, contrastive_inputs, positives  # noqa: F401  (CASES: re-exported for the tests)

REGIMES = {"init": (10.0, -10.0), "mixed": (100.0, -10.0), "linear": (1.0, 0.0)}


def head_of(t, b):
    """The two floats the kernels read: (log t, b)."""
    return torch.tensor([math.log(t), b], dtype=torch.float32)


def sigmoid_ref(q, k, q_group, k_group, head, w, scale=1.0, dtype=torch.float64):
    """The definition in closed form: dict of loss (w * sum), rows [4, R] (row loss, sum of sigmoid - [pos], the same times
    a, best live key index or -1; the index as a float), dq, dk, dhead [2], correct, best [R] (long), the cancellation-free
    scales ``scale_t`` = t sum |G a| and ``scale_b`` = sum |G| (``rows_scale`` [2, R]: sum_j |sigmoid - [pos]| and
    sum_j |(sigmoid - [pos]) a| per row), ``sig`` (the [R, N] sigmoid), ``live``, ``pos`` and ``z`` (dead cells -inf).
    ``dtype=torch.float32``: the same expressions evaluated in fp32, the yardstick of the parity test."""
    q, k = q.detach().to(dtype).cpu(), k.detach().to(dtype).cpu()
    head = head.detach().to(dtype).cpu()
    qg, kg = q_group.cpu().long(), k_group.cpu().long()
    t, b = torch.exp(head[0]), head[1]
    live = (qg[:, None] >= 0) & (kg[None, :] >= 0)
    pos = positives(qg, kg)
    a = q @ k.t()
    z = t * a + b
    sign = torch.where(pos, -torch.ones_like(z), torch.ones_like(z))
    x = sign * z
    cell = x.clamp(min=0) + torch.log1p(torch.exp(-x.abs()))  # softplus without an overflow, its tail kept
    cell = torch.where(live, cell, torch.zeros_like(cell))
    sig = torch.sigmoid(z)
    resid = torch.where(live, sig - pos.to(dtype), torch.zeros_like(sig))
    G = w * scale * resid
    N = z.shape[1]
    zl = z.masked_fill(~live, float("-inf"))
    is_max = (zl == zl.max(dim=1, keepdim=True).values) & live  # ties to the lower j, spelled out
    best = torch.where(is_max, torch.arange(N)[None, :], N).min(dim=1).values
    best = torch.where(best == N, -torch.ones_like(best), best)
    hit = (best >= 0) & pos[torch.arange(len(best)), best.clamp(min=0)]
    rows = torch.stack([cell.sum(1), resid.sum(1), (resid * a).sum(1), best.to(dtype)])
    return dict(loss=w * cell.sum(), rows=rows, dq=t * G @ k, dk=t * G.t() @ q,
                dhead=torch.stack([t * (G * a).sum(), G.sum()]), correct=int(hit.sum()), best=best,
                scale_t=float(t * (G * a).abs().sum()), scale_b=float(G.abs().sum()),
                rows_scale=torch.stack([resid.abs().sum(1), (resid * a).abs().sum(1)]), sig=sig, live=live, pos=pos, z=zl)


def sigmoid_loss(q, k, q_group, k_group, head, w):
    """w * sum of the live cell losses as a differentiable torch expression written from the definition (log(1 + exp) of
    the signed logit through logaddexp), nothing shared with sigmoid_ref: for autograd, ``head`` included."""
    qg, kg = q_group.cpu().long(), k_group.cpu().long()
    live = (qg[:, None] >= 0) & (kg[None, :] >= 0)
    same = qg[:, None] == kg[None, :]
    z = torch.exp(head[0]) * (q @ k.t()) + head[1]
    y = torch.where(same, -z, z)
    return w * torch.logaddexp(y, torch.zeros_like(y))[live].sum()


@functools.lru_cache(maxsize=None)
def sigmoid_case(R, N, d, kind, regime, seed=1):
    """(q, k, q_group, k_group, head, ref, yard) of one case with w = 1 / R, computed once and shared (leave it unchanged):
    the fp64 reference and the fp32 yardstick.  Asserts what keeps the mixed regime mixed: in every case with more than
    one live key at least 5 % of the positive cells and 2 % of the negative cells have a sigmoid in (0.02, 0.98); and,
    where a row has two live keys, a top-1 / top-2 gap of at least 1e-5 t (fp32 must not flip an arg-max)."""
    q, k, qg, kg = contrastive_inputs(R, N, d, kind, seed)
    t, b = REGIMES[regime]
    head = head_of(t, b)
    ref = sigmoid_ref(q, k, qg, kg, head, 1.0 / R)
    yard = sigmoid_ref(q, k, qg, kg, head, 1.0 / R, dtype=torch.float32)
    if int((kg >= 0).sum()) > 1:
        if regime == "mixed":
            mid = (ref["sig"] > 0.02) & (ref["sig"] < 0.98)
            pos, neg = ref["pos"], ref["live"] & ~ref["pos"]
            share_p, share_n = float((mid & pos).sum()) / int(pos.sum()), float((mid & neg).sum()) / int(neg.sum())
            assert share_p >= 0.05 and share_n >= 0.02, (R, N, d, kind, share_p, share_n)
        alive = qg >= 0
        top2 = ref["z"][alive].topk(2, dim=1).values
        gap = float((top2[:, 0] - top2[:, 1]).min())
        assert gap >= 1e-5 * t, (R, N, d, kind, regime, gap)
    return q, k, qg, kg, head, ref, yard
