"""fp64 reference of the multi-positive InfoNCE objective (clipfs_contrastive_objective, include/clipfs.h) and the inputs
its tests share.

Plain random unit vectors at a logit scale of 100 give rows whose loss is ~log N with a softmax spread over a handful of
keys; pulling each query towards the mean of its positives by 0.2 gives mean row losses between ~0.3 and ~11 (a pull of
0.5 saturates the paired 256 x 256 x 512 case to loss 0, where relative gradient errors mean nothing; 0.1 leaves top-1 /
top-2 gaps of 4e-6 s, where fp32 rounding may flip an arg-max).  ``contrastive_case`` asserts the conditions that keep
a test from hiding a failure."""
import functools

import torch

PULL = 0.2

# (R, N, d, kind) of the kernel parity test.  The last two reach the gradient kernel's 512-feature workgroups (four
# accumulators per wave): 4081 is the smallest own side at which a d in (512, 1024] selects them, the first for dq with a
# ragged second feature chunk (600 = 512 + 88), the second for dk.
CASES = [(1, 1, 64, "paired"), (32, 32, 64, "paired"), (33, 65, 64, "groups"), (37, 83, 192, "groups"),
         (256, 256, 512, "paired"), (256, 403, 512, "groups"), (96, 1100, 1024, "groups"), (300, 40, 128, "groups"),
         (4081, 40, 600, "groups"), (40, 4081, 600, "groups")]
# (case, op) pairs whose gradient plan must say feat_chunk == 512
WIDE_GRAD = [((4081, 40, 600, "groups"), "dq"), ((40, 4081, 600, "groups"), "dk")]


def _unit(t):
    return t / t.norm(dim=-1, keepdim=True)


def positives(q_group, k_group):
    """[R, N] bool: key j is a positive of query i (a negative group on either side is never one)."""
    return (q_group[:, None] == k_group[None, :]) & (k_group[None, :] >= 0) & (q_group[:, None] >= 0)


def contrastive_inputs(R, N, d, kind, seed=1):
    """(q [R, d], k [N, d]) fp32 unit rows and int32 groups; one generator per seed, this draw order."""
    g = torch.Generator().manual_seed(seed)
    q = _unit(torch.randn(R, d, generator=g, dtype=torch.float64))
    k = _unit(torch.randn(N, d, generator=g, dtype=torch.float64))
    if kind == "paired":
        assert R == N
        qg = kg = torch.arange(R, dtype=torch.int32)
    else:
        ids = max(2, min(R, N) // 4)
        qg = torch.randint(ids, (R,), generator=g).to(torch.int32)
        kg = torch.randint(ids, (N,), generator=g).to(torch.int32)
        qg[torch.randperm(R, generator=g)[:R // 10]] = -1
        kg[torch.randperm(N, generator=g)[:N // 10]] = -1
    pos = positives(qg, kg).double()
    has = pos.sum(1) > 0
    mean = pos @ k
    mean[has] = _unit(mean[has])
    q = _unit(q + PULL * mean)
    return q.float(), k.float(), qg.clone(), kg.clone()


def contrastive_ref(q, k, q_group, k_group, s, w, scale=1.0, dtype=torch.float64):
    """The definition in fp64, closed form: dict of loss (w * sum), loss_rows [R], dq, dk, n [R], correct and gap (the
    smallest top-1 minus top-2 logit over the rows that have a positive; inf where no row has two live keys).
    ``dtype=torch.float32``: the same expressions evaluated in fp32, the yardstick of the range tests."""
    q, k = q.detach().to(dtype).cpu(), k.detach().to(dtype).cpu()
    qg, kg = q_group.cpu().long(), k_group.cpu().long()
    live = kg >= 0
    pos = positives(qg, kg)
    n = pos.sum(1)
    alive = n > 0
    z = s * q @ k.t()
    zl = z.masked_fill(~live[None, :], float("-inf"))
    lse = torch.logsumexp(zl, dim=1)
    possum = (z * pos).sum(1)
    loss_rows = torch.where(alive, lse - possum / n.clamp(min=1), torch.zeros_like(lse))
    soft = torch.exp(zl - lse[:, None])
    G = w * scale * (soft - pos.to(dtype) / n.clamp(min=1)[:, None].to(dtype))
    G[~alive] = 0
    G[:, ~live] = 0
    is_max = zl == zl.max(dim=1, keepdim=True).values  # ties to the lower j, spelled out: argmax does not promise it
    best = torch.where(is_max, torch.arange(z.shape[1])[None, :], z.shape[1]).min(dim=1).values.clamp(max=z.shape[1] - 1)
    correct = int((alive & pos[torch.arange(len(best)), best]).sum())
    gap = float("inf")
    if int(live.sum()) >= 2 and bool(alive.any()):
        top2 = zl[alive].topk(2, dim=1).values
        gap = float((top2[:, 0] - top2[:, 1]).min())
    return dict(loss=w * loss_rows.sum(), loss_rows=loss_rows, dq=s * G @ k, dk=s * G.t() @ q, n=n, correct=correct, gap=gap,
                alive=alive)


def contrastive_loss(q, k, q_group, k_group, s, w):
    """w * sum of the row losses as a differentiable torch expression (for autograd through a model)."""
    qg, kg = q_group.cpu().long(), k_group.cpu().long()
    live = kg >= 0
    pos = positives(qg, kg)
    n = pos.sum(1)
    alive = n > 0
    z = s * q @ k.t()
    lse = torch.logsumexp(z.masked_fill(~live[None, :], float("-inf")), dim=1)
    rows = lse - (z * pos).sum(1) / n.clamp(min=1)
    return w * rows[alive].sum()


def symmetric_loss(img, txt, img_group, txt_group, s=100.0):
    """1/2 (mean over images of the image -> text loss + mean over captions of the text -> image loss)."""
    return (contrastive_loss(img, txt, img_group, txt_group, s, 0.5 / img.shape[0])
            + contrastive_loss(txt, img, txt_group, img_group, s, 0.5 / txt.shape[0]))


@functools.lru_cache(maxsize=None)
def contrastive_case(R, N, d, kind, s, seed=1):
    """(q, k, q_group, k_group, ref) of one case with w = 1 / R, computed once and shared (leave it unchanged).  Asserts
    the conditions that keep a test honest: the mean row loss in [0.05, 20], at least 3/4 of the rows with a positive,
    top-1 / top-2 gaps of at least 1e-5 s.  With a single live key the loss is identically 0 and there is no second
    logit: the loss and gap conditions have nothing to say about such a case and are not applied to it."""
    q, k, qg, kg = contrastive_inputs(R, N, d, kind, seed)
    ref = contrastive_ref(q, k, qg, kg, s, 1.0 / R)
    assert int(ref["alive"].sum()) * 4 >= 3 * R, (R, N, d, kind, int(ref["alive"].sum()))
    if int((kg >= 0).sum()) > 1:
        mean_loss = float(ref["loss_rows"].mean())
        assert 0.05 <= mean_loss <= 20, (R, N, d, kind, s, mean_loss)
        assert ref["gap"] >= 1e-5 * abs(s), (R, N, d, kind, s, ref["gap"])
    return q, k, qg, kg, ref
