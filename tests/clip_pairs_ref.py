"""fp64 reference of the symmetric CLIP pair objective with a device-side scale (clipfs_clip_pairs_objective,
include/clipfs.h), built from contrastive_ref.contrastive_ref: two calls with the roles swapped, plus the per-row
statistics and dhead = sum G z, which that reference does not return.  Inputs and shapes are the InfoNCE tests'
(contrastive_ref.contrastive_inputs, contrastive_ref.CASES), imported and not copied."""
import functools
import math

import torch

from contrastive_ref import CASES, contrastive_inputs, contrastive_ref, positives  # noqa: F401  (CASES: re-exported)

SCALES = {"100": 100.0, "1/0.07": 1.0 / 0.07, "1": 1.0}
PEAKED = ((37, 83, 192, "groups"), 1000.0)     # one case whose softmax is a single key almost everywhere
ONE_DIRECTIONAL = [(33, 65, 64, "groups"), (256, 403, 512, "groups")]  # also run with weight_k = 0
GAP = 1e-5  # times s: the top-1 / top-2 gap below which fp32 may flip an arg-max


def head_of(s):
    """The float the kernels read: log s, rounded to fp32."""
    return torch.tensor([math.log(s)], dtype=torch.float32)


def _direction(q, k, qg, kg, s, w, scale, dtype):
    """One direction: contrastive_ref's dict plus the statistics rows (lse, 1 / n, loss, E[z] - mean_P z, best index), the
    row gaps and the cancellation-free scales of dhead."""
    ref = contrastive_ref(q, k, qg, kg, s, w, scale, dtype)
    q, k = q.detach().to(dtype).cpu(), k.detach().to(dtype).cpu()
    qg, kg = qg.cpu().long(), kg.cpu().long()
    live = kg >= 0
    pos = positives(qg, kg)
    n = pos.sum(1)
    alive = n > 0
    N = k.shape[0]
    z = s * q @ k.t()
    zl = z.masked_fill(~live[None, :], float("-inf"))
    lse = torch.logsumexp(zl, dim=1)
    g = torch.exp(zl - lse[:, None]) - pos.to(dtype) / n.clamp(min=1)[:, None].to(dtype)  # G without w S
    g[~alive] = 0
    g[:, ~live] = 0
    gz = g * z
    is_max = (zl == zl.max(dim=1, keepdim=True).values) & live[None, :]  # ties to the lower j, spelled out
    best = torch.where(is_max, torch.arange(N)[None, :], N).min(dim=1).values
    best = torch.where((best == N) | (qg < 0), -torch.ones_like(best), best)
    inf = torch.full_like(lse, float("inf"))
    zero = torch.zeros_like(lse)
    rows = torch.stack([torch.where(alive, lse, inf), torch.where(alive, 1.0 / n.clamp(min=1).to(dtype), zero),
                        ref["loss_rows"], gz.sum(1)])
    gaps = torch.full((q.shape[0],), float("inf"), dtype=torch.float64)
    if int(live.sum()) >= 2:
        top2 = zl.topk(2, dim=1).values.double()
        gaps = torch.where(qg >= 0, top2[:, 0] - top2[:, 1], gaps)
    hit = (best >= 0) & pos[torch.arange(len(best)), best.clamp(min=0)]
    ref.update(rows=rows, best=best, hit=hit, gaps=gaps, dz_rows_scale=gz.abs().sum(1), dhead=w * scale * gz.sum(),
               dhead_scale=abs(w) * scale * gz.abs().sum())
    return ref


def clip_pairs_ref(q, k, q_group, k_group, head, weight_q, weight_k=0.0, scale=1.0, dtype=torch.float64):
    """The definition: dict of loss, dq, dk, dhead (and its scale sum |G z|), correct (the two hit counts) and the two
    directions' dicts ``qside`` / ``kside`` (None when weight_k == 0).  s = exp(head[0]) of the fp32 head, evaluated in
    ``dtype``; ``dtype=torch.float32``: the same expressions in fp32, the yardstick of the parity test."""
    s = float(torch.exp(head.detach().cpu().to(dtype)[0]))
    a = _direction(q, k, q_group, k_group, s, weight_q, scale, dtype)
    if weight_k == 0.0:
        return dict(loss=a["loss"], dq=a["dq"], dk=a["dk"], dhead=a["dhead"], dhead_scale=a["dhead_scale"],
                    correct=(a["correct"], 0), qside=a, kside=None, s=s)
    b = _direction(k, q, k_group, q_group, s, weight_k, scale, dtype)
    return dict(loss=a["loss"] + b["loss"], dq=a["dq"] + b["dk"], dk=a["dk"] + b["dq"], dhead=a["dhead"] + b["dhead"],
                dhead_scale=a["dhead_scale"] + b["dhead_scale"], correct=(a["correct"], b["correct"]), qside=a, kside=b, s=s)


@functools.lru_cache(maxsize=None)
def clip_pairs_case(R, N, d, kind, s, both=True, honest=True, seed=1):
    """(q, k, q_group, k_group, head, ref, yard) of one case with the weights 0.5 / R and 0.5 / N (``both=False``: 1 / R
    and 0), computed once and shared (leave it unchanged): the fp64 reference and the fp32 yardstick.  ``honest``: asserts,
    for BOTH directions, the conditions that keep a test from hiding a failure: the mean row loss in [0.05, 20] and at
    least 3/4 of the rows with a positive (a case with a single live key has loss 0 and is not asked).  The arg-max gaps
    are not asserted here: the parity test applies the rule to the rows below GAP s."""
    q, k, qg, kg = contrastive_inputs(R, N, d, kind, seed)
    head = head_of(s)
    wq, wk = (0.5 / R, 0.5 / N) if both else (1.0 / R, 0.0)
    ref = clip_pairs_ref(q, k, qg, kg, head, wq, wk)
    yard = clip_pairs_ref(q, k, qg, kg, head, wq, wk, dtype=torch.float32)
    if honest:
        for side, rows, other in ((ref["qside"], R, kg), (ref["kside"], N, qg)):
            if side is None:
                continue
            assert int(side["alive"].sum()) * 4 >= 3 * rows, (R, N, d, kind, int(side["alive"].sum()), rows)
            if int((other >= 0).sum()) > 1:
                mean_loss = float(side["loss_rows"].mean())
                assert 0.05 <= mean_loss <= 20, (R, N, d, kind, s, mean_loss)
    return q, k, qg, kg, head, ref, yard
