"""Training-free kernel ridge regression head (ProKeR: Bendou et al., "ProKeR: A Kernel Perspective on Few-Shot
Adaptation of Large Vision-Language Models", CVPR 2025) on the HIP engine: the Tip-Adapter kernel
k(x, s) = exp(-beta (1 - x . s)) with the global, closed-form solution of the ridge problem in its RKHS, regularised
towards the zero-shot predictor,

    logits(x) = clip_logits(x) + k(x, S) (k(S, S) + lam I)^-1 (target_scale * onehot(Y) - shot_logits)

    ProKeRHead       the head: the n x n system built, factored and solved on the device (csrc/krr.hip on the Cholesky
                     layer of csrc/spd.hip: the fused pair up to 1024 shots, the panelled pair up to 16384), applied with
                     ONE launch that never writes the [B, n] affinity
    search_hp        a (beta, lam) grid search: a plain LOOP of fits and applies, one host read at the end
    evaluate_proker  top-1 before and after

It starts from the same (features, labels) that ``tip_adapter.collect_features`` produces, in any label order, and sits on
features only, so it composes with ViT or ModifiedResNet towers, LoRA-tuned or merged models; features in any precision
mode are taken as fp32.  The rule is written out in include/clipfs.h ("KRR") and is the contract; it is more general than
the paper in the caller-supplied base logits and the target scale.  There is no CPU path.
Not offered: backward / training of the keys, leave-one-out lambda selection, iterative refinement, data parallelism,
fp16 storage, n above 16 384, a normalised (Nadaraya-Watson) variant.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from clipfs import ops


class ProKeRHead(nn.Module):
    """The head.  Buffers ``shots`` [n, d] (the keys), ``At`` [C, n4] (the solution, one class per row, n4 = n rounded up
    to 4, pad columns 0) and ``info`` int32 [1] (the factor's: 0, or the first pivot that was not positive).  ``beta``,
    ``lam``, ``target_scale`` and ``panel`` are plain values; they travel in the state dict."""

    def __init__(self, shots: torch.Tensor, At: torch.Tensor, info: torch.Tensor, beta: float = 5.5, lam: float = 1.0,
                 target_scale: float = 1.0, panel: int = 256):
        super().__init__()
        assert shots.dim() == 2 and At.dim() == 2 and At.shape[1] == (shots.shape[0] + 3) // 4 * 4
        self.register_buffer("shots", shots.float().contiguous())
        self.register_buffer("At", At.float().contiguous())
        self.register_buffer("info", info.to(torch.int32).contiguous())
        self.beta, self.lam, self.target_scale, self.panel = float(beta), float(lam), float(target_scale), int(panel)

    @classmethod
    def from_features(cls, features: torch.Tensor, labels: torch.Tensor, n_classes: int,
                      shot_logits: Optional[torch.Tensor] = None, beta: float = 5.5, lam: float = 1.0,
                      target_scale: float = 1.0, panel: int = 256) -> "ProKeRHead":
        """The head of ``features`` [n, d] (unit rows, on the GPU) with ``labels`` [n] in [0, n_classes), in any order;
        ``shot_logits`` [n, C]: the base predictor's logits of the shots (None: 0)."""
        if not features.is_cuda:
            raise ValueError("ProKeRHead.from_features: the features must be on the GPU (there is no CPU path)")
        if features.dim() != 2 or labels.shape != (features.shape[0],) or not 1 <= features.shape[0] <= 16384:
            raise ValueError(f"from_features: features {tuple(features.shape)} with labels {tuple(labels.shape)} (1 <= n <= 16384)")
        if features.shape[1] % 4 or not 4 <= features.shape[1] <= 1024:
            raise ValueError(f"from_features: the feature width {features.shape[1]} must be a multiple of 4 in [4, 1024]")
        host = labels.detach().to("cpu", torch.int32).contiguous()
        if n_classes < 1 or int(host.min()) < 0 or int(host.max()) >= n_classes:
            raise ValueError(f"from_features: labels outside [0, {n_classes})")
        shots = features.float().contiguous()
        base = None if shot_logits is None else shot_logits.to(features.device).float()
        out = ops.krr_fit(shots, host.to(features.device), n_classes, base, beta, lam, target_scale, panel, labels_host=host)
        return cls(shots, out["At"], out["info"], beta, lam, target_scale, panel)

    @property
    def n_classes(self) -> int:
        return self.At.shape[0]

    def factor_info(self) -> int:
        """The Cholesky factor's ``info`` (this reads the device: it synchronises): 0, or the 1-based index of the first
        pivot that was <= 0 or not finite, in which case ``At`` holds nothing to rely on."""
        return int(self.info.item())

    @torch.no_grad()
    def forward(self, features: torch.Tensor, clip_logits: Optional[torch.Tensor] = None) -> torch.Tensor:
        """logits [B, C] = clip_logits + k(features, shots) At^T for unit ``features`` [B, d] (never normalised here);
        ``clip_logits`` None: 0.  One launch."""
        if not (features.is_cuda and self.At.is_cuda):
            raise ValueError("ProKeRHead: the head and the features must be on the GPU (there is no CPU path)")
        if features.dim() != 2 or features.shape[1] != self.shots.shape[1]:
            raise ValueError(f"ProKeRHead: features {tuple(features.shape)} for a head of width {self.shots.shape[1]}")
        base = None if clip_logits is None else clip_logits.float()
        return ops.krr_apply(features.float().contiguous(), self.shots, self.At, base, self.beta)

    def get_extra_state(self):
        return {"beta": self.beta, "lam": self.lam, "target_scale": self.target_scale, "panel": self.panel}

    def set_extra_state(self, state) -> None:
        self.beta, self.lam = float(state["beta"]), float(state["lam"])
        self.target_scale, self.panel = float(state["target_scale"]), int(state["panel"])


@torch.no_grad()
def search_hp(features: torch.Tensor, labels: torch.Tensor, n_classes: int, shot_logits: Optional[torch.Tensor],
              val_features: torch.Tensor, val_logits: Optional[torch.Tensor], val_target: torch.Tensor,
              betas: Sequence[float], lams: Sequence[float], target_scale: float = 1.0,
              panel: int = 256) -> Tuple[float, float, torch.Tensor]:
    """Top-1 hits on the validation set of every (beta, lam) cell.  This is a plain LOOP: one fit and one apply per
    cell (the system depends on both), the hit counts stay on the device and are read once at the end; the first
    maximum in (beta-major, lam-minor) order wins, ties inside a row going to the lower class.  Returns
    (beta, lam, hits int32 [len(betas), len(lams)])."""
    if not len(betas) or not len(lams):
        raise ValueError("search_hp: an empty grid")
    dev = features.device
    target = val_target.to(dev).long().contiguous()
    one = torch.ones(1, device=dev, dtype=torch.float32)
    cells = []
    for beta in betas:
        for lam in lams:
            head = ProKeRHead.from_features(features, labels, n_classes, shot_logits, float(beta), float(lam), target_scale, panel)
            cells.append(ops.gda_search(head(val_features, val_logits), None, target, one))  # argmax, ties to the lower class
    hits = torch.cat(cells).reshape(len(betas), len(lams))
    best = int(np.argmax(hits.cpu().numpy()))  # numpy: the first maximum; the one host read
    return float(betas[best // len(lams)]), float(lams[best % len(lams)]), hits


@torch.no_grad()
def evaluate_proker(model, head: ProKeRHead, loader) -> dict:
    """Top-1 accuracy of the zero-shot logits alone and with the head on top, over ``loader`` (batches of
    (images, target)); ``model`` maps images to (unit features [B, d], clip_logits [B, C]).  dict(zero_shot, proker, n)."""
    dev = head.At.device
    zs = torch.zeros((), device=dev, dtype=torch.int64)
    pk = torch.zeros((), device=dev, dtype=torch.int64)
    n = 0
    for batch in loader:
        images, target = (batch[0], batch[1]) if len(batch) == 2 else (batch[0], batch[2])
        feats, logits = model(images.to(dev))
        target = target.to(dev).long()
        zs += (logits.argmax(1) == target).sum()
        pk += (head(feats, logits).argmax(1) == target).sum()
        n += int(target.numel())
    return {"zero_shot": float(zs.item()) / max(n, 1), "proker": float(pk.item()) / max(n, 1), "n": n}
