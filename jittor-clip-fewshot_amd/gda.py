"""Training-free Gaussian discriminant head (Wang et al., "A Hard-to-Beat Baseline for Training-Free CLIP-Based
Adaptation", ICLR 2024) on the HIP engine: one mean per class and ONE shared full covariance of the few-shot features,
shrunk towards its trace, in closed form,

    W = d * ((M - 1) Sigma + shrink * trace(Sigma) I)^-1 mu,   b_c = log pi_c - 1/2 mu_c . W_c
    logits = clip_logits + alpha * (f W^T + b)

    GDAHead        the head: built from features in 6 + ceil(d / 32) launches (csrc/gda.hip on the Cholesky factor and
                   solve of csrc/spd.hip), applied with ONE fused GEMM launch
    search_alpha   the alpha grid search every user of the method runs, in one launch
    evaluate_gda   top-1 before and after

It starts from the same (features, labels) that ``tip_adapter.collect_features`` produces and sits on features only, so it
composes with ViT or ModifiedResNet towers, LoRA-tuned or merged models.  The rule is written out in include/clipfs.h
("GDA") and is the contract.  There is no CPU path.
Not offered: classes without shots, per-class covariances, training W, data parallelism, fp16 storage, feature widths
above 1024 (the factor's limit).
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from clipfs import ops


class GDAHead(nn.Module):
    """The head.  Buffers ``W`` [C, d], ``b`` [C], ``mu`` [C, d], ``offsets`` int32 [C + 1] (class c owned shots
    offsets[c] .. offsets[c + 1] - 1 of the sorted features) and ``info`` int32 [1] (the factor's: 0, or the first
    pivot that was not positive).  ``alpha``, ``prior`` and ``shrink`` are plain values; they travel in the state dict."""

    def __init__(self, W: torch.Tensor, b: torch.Tensor, mu: torch.Tensor, offsets: torch.Tensor, info: torch.Tensor,
                 alpha: float = 1.0, prior: str = "uniform", shrink: float = 1.0):
        super().__init__()
        assert W.dim() == 2 and W.shape == mu.shape and b.shape == (W.shape[0],) and offsets.dtype == torch.int32
        self.register_buffer("W", W.float().contiguous())
        self.register_buffer("b", b.float().contiguous())
        self.register_buffer("mu", mu.float().contiguous())
        self.register_buffer("offsets", offsets.contiguous())
        self.register_buffer("info", info.to(torch.int32).contiguous())
        self.alpha, self.prior, self.shrink = float(alpha), str(prior), float(shrink)

    @classmethod
    def from_features(cls, features: torch.Tensor, labels: torch.Tensor, n_classes: int, prior: str = "uniform",
                      shrink: float = 1.0, alpha: float = 1.0) -> "GDAHead":
        """The head of ``features`` [M, d] (unit rows, on the GPU) with ``labels`` [M] in [0, n_classes): a stable sort by
        label, then ``ops.gda_fit``.  Every class needs at least one shot."""
        if not features.is_cuda:
            raise ValueError("GDAHead.from_features: the features must be on the GPU (there is no CPU path)")
        labels = labels.to(features.device).long()
        if features.dim() != 2 or labels.shape != (features.shape[0],) or features.shape[0] < 2:
            raise ValueError(f"from_features: features {tuple(features.shape)} with labels {tuple(labels.shape)} (M >= 2)")
        if features.shape[1] % 4 or not 4 <= features.shape[1] <= 1024:
            raise ValueError(f"from_features: the feature width {features.shape[1]} must be a multiple of 4 in [4, 1024]")
        if n_classes < 1 or int(labels.min()) < 0 or int(labels.max()) >= n_classes:
            raise ValueError(f"from_features: labels outside [0, {n_classes})")
        sorted_labels, order = torch.sort(labels, stable=True)
        counts = torch.bincount(sorted_labels, minlength=n_classes)
        offsets = torch.zeros(n_classes + 1, dtype=torch.int32, device=features.device)
        offsets[1:] = torch.cumsum(counts, 0).to(torch.int32)
        host = offsets.cpu()
        empty = np.flatnonzero(np.diff(host.numpy()) == 0)
        if empty.size:
            raise ValueError(f"from_features: class {int(empty[0])} has no shot (classes without shots are not offered)")
        shots = features.float().index_select(0, order).contiguous()
        out = ops.gda_fit(shots, offsets, prior=prior, shrink=shrink, offsets_host=host)
        return cls(out["W"], out["b"], out["mu"], offsets, out["info"], alpha, prior, shrink)

    @property
    def n_classes(self) -> int:
        return self.offsets.numel() - 1

    def factor_info(self) -> int:
        """The Cholesky factor's ``info`` (this reads the device: it synchronises): 0, or the 1-based index of the first
        pivot that was <= 0 or not finite, in which case W and b are not numbers to rely on."""
        return int(self.info.item())

    @torch.no_grad()
    def scores(self, features: torch.Tensor) -> torch.Tensor:
        """g = f W^T + b [B, C]: what the head adds per unit of alpha."""
        self._check(features)
        return ops.gemm_nt(features.float().contiguous(), self.W, bias=self.b, split_k=False)

    @torch.no_grad()
    def forward(self, features: torch.Tensor, clip_logits: Optional[torch.Tensor] = None) -> torch.Tensor:
        """logits [B, C] = clip_logits + alpha (f W^T + b) for unit ``features`` [B, d] (never normalised here);
        ``clip_logits`` None: 0.  One GEMM launch with the bias and the residual in its epilogue."""
        self._check(features)
        res = None if clip_logits is None else clip_logits.float().contiguous()
        return ops.gemm_nt(features.float().contiguous(), self.W, alpha=self.alpha, bias=self.b * self.alpha, residual=res,
                           split_k=False)

    def _check(self, features: torch.Tensor) -> None:
        if not (features.is_cuda and self.W.is_cuda):
            raise ValueError("GDAHead: the head and the features must be on the GPU (there is no CPU path)")
        if features.dim() != 2 or features.shape[1] != self.W.shape[1]:
            raise ValueError(f"GDAHead: features {tuple(features.shape)} for a head of width {self.W.shape[1]}")

    def get_extra_state(self):
        return {"alpha": self.alpha, "prior": self.prior, "shrink": self.shrink}

    def set_extra_state(self, state) -> None:
        self.alpha, self.prior, self.shrink = float(state["alpha"]), str(state["prior"]), float(state["shrink"])


@torch.no_grad()
def search_alpha(head: GDAHead, features: torch.Tensor, clip_logits: Optional[torch.Tensor], target: torch.Tensor,
                 alphas: Optional[Sequence[float]] = None) -> Tuple[float, torch.Tensor]:
    """Top-1 hits of every alpha of the grid (default 1e-4 ... 1e4 in powers of ten) in one launch on g = f W^T + b,
    formed once; sets the first maximum on the head.  Returns (alpha, hits int32 [nA])."""
    dev = head.W.device
    values = ops.GDA_DEFAULT_ALPHAS if alphas is None else alphas
    a = values if torch.is_tensor(values) else torch.tensor([float(v) for v in values], dtype=torch.float32)
    a = a.detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
    if a.numel() < 1:
        raise ValueError("search_alpha: an empty grid")
    g = head.scores(features)
    base = None if clip_logits is None else clip_logits.float()
    hits = ops.gda_search(g, base, target.to(dev).long().contiguous(), a)
    best = int(np.argmax(hits.cpu().numpy()))  # numpy: the first maximum
    head.alpha = float(a[best])
    return head.alpha, hits


@torch.no_grad()
def evaluate_gda(head: GDAHead, features: torch.Tensor, clip_logits: torch.Tensor, target: torch.Tensor) -> dict:
    """Top-1 accuracy of ``clip_logits`` alone and with the head on top (at ``head.alpha``): dict(zero_shot, gda, n)."""
    target = target.to(head.W.device).long()
    n = int(target.numel())
    with_head = head(features, clip_logits)
    return {"zero_shot": float((clip_logits.argmax(1) == target).sum().item()) / n,
            "gda": float((with_head.argmax(1) == target).sum().item()) / n, "n": n}
