"""Tip-Adapter cache head (Zhang et al., "Tip-Adapter: Training-free Adaption of CLIP for Few-shot Classification",
ECCV 2022) on the HIP engine: a key-value cache over the few-shot features with one-hot values,

    logits = clip_logits + alpha * sum over the keys k of a class of exp(-beta (1 - f . K[k]))

    collect_features   the cache keys: unit image features of a pool, averaged over augmentation epochs
    TipAdapter         the head (training-free as built; ``keys`` is its one Parameter)
    search_hp          the alpha / beta grid search every user of the method runs, in ONE launch
    TipAdapterTrainer  Tip-Adapter-F: trains the keys only (flat fp32 buffers, one AdamW launch per step)

The head sits on features only, so it composes with ViT or ModifiedResNet towers, LoRA-tuned or merged models and MTA
mode features.  The kernels (csrc/cache_head.hip) keep the [B, NK] affinity on chip and are deterministic; the keys
are kept SORTED BY CLASS, which is what lets a class's cache term be a run sum and the search keep nothing of size C.
Not offered: soft or learned cache values, training alpha / beta, data parallelism, loss scaling, EMA.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from clipfs import ops


@torch.no_grad()
def collect_features(clip_model, loader, epochs: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """(features [N, d] unit rows, labels [N] int64) of the loader's pool, row i = pool image i: each image's unit
    ``encode_image`` features summed over ``epochs`` augmentation passes of ``loader`` (a ``clipfs.data.TrainLoader``:
    batches ``(images, raw, target, index)``), divided by ``epochs`` and renormalised.  Each index occurs once per epoch
    (``drop_last`` must be off), so an image's sum runs in epoch order whatever the shuffle: the result is
    deterministic."""
    if epochs < 1:
        raise ValueError(f"collect_features: epochs = {epochs}")
    if getattr(loader, "drop_last", False):
        raise ValueError("collect_features: the loader drops the last batch, so some pool images would get no feature")
    n = len(loader.pool)
    acc = None
    for _ in range(epochs):
        for images, _raw, _target, index in loader:
            if images is None:
                raise ValueError("collect_features: the loader must yield the 'clip' output")
            f = ops.l2norm_fwd(clip_model.encode_image(images).float().contiguous())
            if acc is None:
                acc = torch.zeros(n, f.shape[1], device=f.device, dtype=torch.float32)
            acc.index_copy_(0, index, acc.index_select(0, index) + f)  # unique indices: no atomics, one writer per row
    if acc is None:
        raise ValueError("collect_features: the loader yielded no batch")
    acc.mul_(1.0 / epochs)
    return ops.l2norm_fwd(acc), loader.pool.labels.clone()


class TipAdapter(nn.Module):
    """The cache head.  ``keys`` [NK, d] (Parameter, sorted by class), ``labels`` [NK] int64 (ascending), ``offsets``
    int32 [C + 1] (class c owns keys offsets[c] .. offsets[c + 1] - 1; a class may own none) and ``order`` [NK] int64
    (``keys[i]`` was row ``order[i]`` of the caller's features).  ``alpha`` / ``beta`` are plain floats (not trained);
    they travel in the state dict."""

    def __init__(self, keys: torch.Tensor, labels: torch.Tensor, offsets: torch.Tensor, order: torch.Tensor,
                 alpha: float = 1.0, beta: float = 5.5):
        super().__init__()
        assert keys.dim() == 2 and labels.shape == order.shape == (keys.shape[0],) and offsets.dtype == torch.int32
        self.keys = nn.Parameter(keys.detach().float().contiguous().clone())
        self.register_buffer("labels", labels.long().contiguous())
        self.register_buffer("offsets", offsets.contiguous())
        self.register_buffer("order", order.long().contiguous())
        self.alpha, self.beta = float(alpha), float(beta)

    @classmethod
    def from_features(cls, features: torch.Tensor, labels: torch.Tensor, n_classes: int, alpha: float = 1.0,
                      beta: float = 5.5) -> "TipAdapter":
        """Cache of ``features`` [NK, d] (unit rows) with ``labels`` [NK] in [0, n_classes): a stable sort by label."""
        labels = labels.to(features.device).long()
        if features.dim() != 2 or labels.shape != (features.shape[0],) or features.shape[0] < 1:
            raise ValueError(f"from_features: features {tuple(features.shape)} with labels {tuple(labels.shape)}")
        if features.shape[1] % 4 or not 4 <= features.shape[1] <= 4096:
            raise ValueError(f"from_features: the feature width {features.shape[1]} must be a multiple of 4 in [4, 4096]")
        if n_classes < 1 or int(labels.min()) < 0 or int(labels.max()) >= n_classes:
            raise ValueError(f"from_features: labels outside [0, {n_classes})")
        sorted_labels, order = torch.sort(labels, stable=True)
        counts = torch.bincount(sorted_labels, minlength=n_classes)
        offsets = torch.zeros(n_classes + 1, dtype=torch.int32, device=features.device)
        offsets[1:] = torch.cumsum(counts, 0).to(torch.int32)
        return cls(features.index_select(0, order), sorted_labels, offsets, order, alpha, beta)

    @property
    def n_classes(self) -> int:
        return self.offsets.numel() - 1

    def forward(self, features: torch.Tensor, clip_logits: Optional[torch.Tensor] = None) -> torch.Tensor:
        """logits [B, C] for unit ``features`` [B, d] (never normalised here) on top of ``clip_logits`` [B, C] (None: 0).
        Differentiable w.r.t. the keys, the clip logits and, when they require grad, the features."""
        return ops.CacheLogitsFn.apply(features.float(), self.keys, self.offsets, clip_logits, self.alpha, self.beta)

    def get_extra_state(self):
        return {"alpha": self.alpha, "beta": self.beta}

    def set_extra_state(self, state) -> None:
        self.alpha, self.beta = float(state["alpha"]), float(state["beta"])


def _grid(values, device) -> torch.Tensor:
    t = values if torch.is_tensor(values) else torch.tensor([float(v) for v in values], dtype=torch.float32)
    t = t.detach().to(device=device, dtype=torch.float32).reshape(-1).contiguous()
    if t.numel() < 1:
        raise ValueError("search_hp: an empty grid")
    return t


@torch.no_grad()
def search_hp(adapter: TipAdapter, features: torch.Tensor, clip_logits: Optional[torch.Tensor], target: torch.Tensor,
              alphas: Sequence[float], betas: Sequence[float]):
    """Top-1 hits of every (beta, alpha) cell in one launch; sets the first maximum in beta-major order
    (``for beta: for alpha:`` with a strict ``>``) on the adapter.  Returns (alpha, beta, hits int32 [nB, nA])."""
    dev = adapter.keys.device
    a, b = _grid(alphas, dev), _grid(betas, dev)
    hits = ops.cache_search(features.float().contiguous(), adapter.keys.detach(), adapter.offsets, clip_logits,
                            target.to(dev).long().contiguous(), a, b)
    best = int(np.argmax(hits.cpu().numpy().reshape(-1)))  # numpy: the first maximum of the row-major walk
    j, i = divmod(best, a.numel())
    adapter.alpha, adapter.beta = float(a[i]), float(b[j])
    return adapter.alpha, adapter.beta, hits


class TipAdapterTrainer:
    """Tip-Adapter-F: AdamW on the cache keys alone (no re-normalisation of the keys, as the method trains them).

    Keys, gradient and both moments live in flat fp32 buffers (``adapter.keys`` becomes a view of the first); a step is
    the logits launch, the one cross-entropy kernel, the key-gradient launch and ONE ``ops.adamw_ext`` launch at the
    pre-step learning rate, then the cosine schedule (``slow_pace.CosineAnnealingLR``, with ``T_max``) advances.  ``step``
    never synchronises with the host.  It stands alone: no engine, no model, no data parallelism, loss scaling or EMA."""

    def __init__(self, adapter: TipAdapter, lr: float = 1e-3, weight_decay: float = 1e-2, betas=(0.9, 0.999),
                 eps: float = 1e-4, T_max: Optional[int] = None):
        if not adapter.keys.is_cuda:
            raise ValueError("TipAdapterTrainer: the adapter must be on the GPU (there is no CPU path)")
        self.adapter = adapter
        self.params = adapter.keys.detach().clone().contiguous().view(-1)
        adapter.keys.data = self.params.view_as(adapter.keys)
        self.grads = torch.zeros_like(self.params)
        self.m = torch.zeros_like(self.params)
        self.v = torch.zeros_like(self.params)
        self.lr, self.wd, self.betas, self.eps = float(lr), float(weight_decay), tuple(betas), float(eps)
        self.t = 0
        self.sched = None
        if T_max is not None:
            from slow_pace import CosineAnnealingLR
            self.sched = CosineAnnealingLR(self.lr, T_max)

    def step(self, features: torch.Tensor, clip_logits: Optional[torch.Tensor], target: torch.Tensor):
        """One optimiser step on a batch of unit ``features`` [B, d]: returns (loss_sum [1] fp32, correct [1] int32),
        device tensors (mean cross entropy = loss_sum / B)."""
        ad = self.adapter
        f = features.detach().float().contiguous()
        keys = self.params.view_as(ad.keys)
        logits = ops.cache_logits(f, keys, ad.offsets, clip_logits, ad.alpha, ad.beta)
        loss_sum, dlogits, correct = ops.cross_entropy(logits, target)
        self.grads.zero_()
        ops.cache_bwd(f, keys, ad.offsets, dlogits, self.grads.view_as(ad.keys), ad.alpha, ad.beta)
        self.t += 1
        ops.adamw_ext(self.params, self.grads, self.m, self.v, self.t, self.lr, self.betas, self.eps, self.wd)
        if self.sched is not None:
            self.lr = self.sched.step()
        return loss_sum, correct

    def state_dict(self) -> dict:
        """Everything a bit-for-bit resume needs (tensors are clones)."""
        s = self.sched
        return {"params": self.params.clone(), "m": self.m.clone(), "v": self.v.clone(), "t": int(self.t),
                "lr": float(self.lr), "alpha": self.adapter.alpha, "beta": self.adapter.beta,
                "hyper": {"weight_decay": self.wd, "betas": tuple(self.betas), "eps": self.eps},
                "scheduler": None if s is None else {"base_lr": s.base_lr, "T_max": s.T_max, "eta_min": s.eta_min,
                                                     "last_epoch": s.last_epoch}}

    def load_state_dict(self, sd: dict) -> None:
        if sd["params"].numel() != self.params.numel():
            raise ValueError(f"the saved state holds {sd['params'].numel()} key elements, this cache {self.params.numel()}")
        if (self.sched is None) != (sd["scheduler"] is None):
            raise ValueError("the saved state " + ("has no" if self.sched is not None else "carries a")
                             + " scheduler position: the trainer was built with another T_max setting")
        for dst, key in ((self.params, "params"), (self.m, "m"), (self.v, "v")):
            dst.copy_(sd[key])
        self.t, self.lr = int(sd["t"]), float(sd["lr"])
        self.adapter.alpha, self.adapter.beta = float(sd["alpha"]), float(sd["beta"])
        h = sd["hyper"]
        self.wd, self.betas, self.eps = float(h["weight_decay"]), tuple(h["betas"]), float(h["eps"])
        if self.sched is not None:
            s = sd["scheduler"]
            self.sched.base_lr, self.sched.T_max = float(s["base_lr"]), int(s["T_max"])
            self.sched.eta_min, self.sched.last_epoch = float(s["eta_min"]), int(s["last_epoch"])
