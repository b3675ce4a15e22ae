"""Training-free dynamic adapter (Karmanov et al., "Efficient Test-Time Adaptation of Vision-Language Models", CVPR 2024)
on the HIP engine: a zero-shot classifier adapted while it runs, from unlabelled test images, with no backward pass and no
extra views.  One feature per image feeds two small caches:

    positive cache   per class a queue of the lowest-entropy test features seen so far, pseudo-labelled by CLIP's own
                     prediction; it ADDS ``pos_alpha exp(-pos_beta (1 - f . k))`` to the logit of the key's class
    negative cache   for medium-entropy samples, the feature with a mask of the classes the sample is probably NOT; it
                     SUBTRACTS ``neg_alpha exp(-neg_beta (1 - f . k))`` from the masked logits

    TestTimeDynamicAdapter   the caches (fixed-shape device tensors) and the ``adapt_*`` calls
    TDAResult                what an ``adapt_*`` call returns
    evaluate_tda             top-1 accuracy of a loader with and without the caches

The rule (include/clipfs.h, "TDA") is the published one-sample-at-a-time rule, and a call over B samples IS B applications
of it in row order: ``ops.tda_adapt`` (csrc/tda.hip) turns the queue updates into intervals with one thread per class and
the logits into a dense masked sum, at most five launches whatever B and C, no host synchronisation, bitwise equal run to
run.  A sample's prediction, entropy and mask do not depend on the batch around it, so a stream gives the same caches
however it is cut into calls.

``adapt_views`` / ``adapt_view_features`` put the paper's multi-view front end before the caches: of the V views of an image
(``clipfs.augmix.view_groups``: AugMix views made on the device) the ``max(1, int(V rho))`` most confident ones are kept and
the mean of their unit features is the image's one feature.

Not offered: sharing a cache among data-parallel ranks (each rank's stream adapts on its own), hyper-parameter search.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from clipfs import ops

MAX_BATCH = ops.TDA_MAX_BATCH  # of clipfs_tda_adapt; longer streams are fed in chunks (exact by the batch contract)
_STATE = ("pos_keys", "pos_ent", "pos_seq", "neg_keys", "neg_ent", "neg_seq", "neg_mask", "counter")


class TDAResult(NamedTuple):
    logits: torch.Tensor        # [B, C]  the adapted logits
    clip_pred: torch.Tensor     # [B] int32  CLIP's own prediction (argmax of the zero-shot logits, ties to the lower index)
    entropy: torch.Tensor       # [B]  entropy of the zero-shot softmax, nats
    pos_inserted: torch.Tensor  # [B] bool  the sample entered the positive cache
    neg_inserted: torch.Tensor  # [B] bool  ... the negative cache


class TestTimeDynamicAdapter:
    """The two caches over ``n_classes`` classes.  Class features: ``text_features`` [C, d] (normalised here), or
    ``clip_model`` plus ``class_features`` [C, d] / ``tokenized_prompts`` [C, L] (encoded once with ``encode_text``);
    ``clip_model`` is also what ``adapt_images`` runs.  Hyper-parameters are those of ``ops.TDA_DEFAULTS`` (logit_scale 100,
    pos_cap 3, neg_cap 2, pos_alpha 2, pos_beta 5, neg_alpha 0.117, neg_beta 1, entropy band (0.2, 0.5), mask band
    (0.03, 1)); a capacity of 0 disables that cache.

    ValueError for an unknown hyper-parameter, a capacity outside [0, 8], class features that are not [n_classes, d]."""

    __test__ = False  # not a test class, whatever the name says to a collector

    def __init__(self, text_features: Optional[torch.Tensor] = None, *, clip_model=None, class_features=None,
                 tokenized_prompts=None, n_classes: Optional[int] = None, device=None, **hyper):
        unknown = sorted(set(hyper) - set(ops.TDA_DEFAULTS))
        if unknown:
            raise ValueError(f"TestTimeDynamicAdapter: unknown hyper-parameter(s) {', '.join(unknown)}; known: "
                             f"{', '.join(sorted(ops.TDA_DEFAULTS))}")
        self.hyper = {**ops.TDA_DEFAULTS, **hyper}
        for cap in ("pos_cap", "neg_cap"):
            if int(self.hyper[cap]) != self.hyper[cap] or not 0 <= self.hyper[cap] <= 8:
                raise ValueError(f"TestTimeDynamicAdapter: {cap} = {self.hyper[cap]} must be an integer in [0, 8]")
            self.hyper[cap] = int(self.hyper[cap])
        self.model = clip_model
        feats = text_features if text_features is not None else class_features
        if feats is None:
            if clip_model is None or tokenized_prompts is None:
                raise ValueError("TestTimeDynamicAdapter: give text_features, or clip_model with class_features or "
                                 "tokenized_prompts")
            with torch.no_grad():
                feats = clip_model.encode_text(tokenized_prompts.to(clip_model.device))
        if device is None:
            device = clip_model.device if clip_model is not None else feats.device
        feats = feats.detach().to(device=device, dtype=torch.float32).contiguous()
        if feats.dim() != 2 or (n_classes is not None and feats.shape[0] != n_classes):
            raise ValueError(f"TestTimeDynamicAdapter: class features {tuple(feats.shape)} are not [n_classes = {n_classes}, d]")
        self.text = ops.l2norm_fwd(feats)
        self.n_classes, self.width = self.text.shape
        self.device = self.text.device
        self.reset()

    # ------------------------------------------------------------------------------------------------ state
    def reset(self) -> None:
        """Empty caches, sample counter 0."""
        self.state = ops.tda_new_state(self.n_classes, self.width, self.hyper["pos_cap"], self.hyper["neg_cap"], self.device)

    def _meta(self) -> dict:
        return dict(n_classes=self.n_classes, width=self.width, **self.hyper)

    def state_dict(self) -> dict:
        """CPU tensors and plain values: the caches, the counter and what they were built for."""
        return {"meta": self._meta(), **{k: self.state[k].detach().cpu().clone() for k in _STATE}}

    def load_state_dict(self, sd: dict) -> None:
        """Refuses (ValueError naming the field) a state made for another C, d, capacity or hyper-parameter set."""
        meta, own = sd.get("meta"), self._meta()
        if not isinstance(meta, dict):
            raise ValueError("TestTimeDynamicAdapter.load_state_dict: no 'meta' record")
        for k, v in own.items():
            if k not in meta or meta[k] != v:
                raise ValueError(f"TestTimeDynamicAdapter.load_state_dict: the state was made for {k} = {meta.get(k)!r}, "
                                 f"this adapter has {k} = {v!r}")
        for k in _STATE:
            t = sd.get(k)
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(self.state[k].shape) or t.dtype != self.state[k].dtype:
                raise ValueError(f"TestTimeDynamicAdapter.load_state_dict: {k} is missing or not a {self.state[k].dtype} "
                                 f"tensor of shape {tuple(self.state[k].shape)}")
        for k in _STATE:
            self.state[k].copy_(sd[k])

    # ------------------------------------------------------------------------------------------------ adapt
    @torch.no_grad()
    def adapt_features(self, feats: torch.Tensor, update: bool = True) -> TDAResult:
        """``feats`` [B, d] unit image features, in stream order.  ``update=False`` scores against the caches as they stand
        and changes nothing.  Never synchronises with the host."""
        if feats.dim() != 2 or feats.shape[1] != self.width:
            raise ValueError(f"adapt_features: expected feats [B, {self.width}], got {tuple(feats.shape)}")
        feats = feats.detach().to(device=self.device, dtype=torch.float32).contiguous()
        B = feats.shape[0]
        hyper = {k: v for k, v in self.hyper.items() if k not in ("pos_cap", "neg_cap")}
        if B <= MAX_BATCH:
            logits, rec = ops.tda_adapt(feats, self.text, self.state, update, **hyper)
            return self._result(logits, rec)
        logits = torch.empty(B, self.n_classes, device=self.device, dtype=torch.float32)
        parts = []
        for b0 in range(0, B, MAX_BATCH):
            _, rec = ops.tda_adapt(feats[b0:b0 + MAX_BATCH], self.text, self.state, update, out=logits[b0:b0 + MAX_BATCH],
                                   **hyper)
            parts.append(self._result(None, rec))
        return TDAResult(logits, *(torch.cat([p[i] for p in parts]) for i in range(1, 5)))

    @staticmethod
    def _result(logits, rec) -> TDAResult:
        return TDAResult(logits, rec["pred"], rec["entropy"], rec["pos_slot"] >= 0, rec["neg_slot"] >= 0)

    @torch.no_grad()
    def adapt_images(self, images: torch.Tensor, update: bool = True) -> TDAResult:
        """Image tower forward (ViT or ModifiedResNet, any precision mode), normalisation, then ``adapt_features``."""
        if self.model is None:
            raise ValueError("adapt_images: the adapter was built without a clip_model")
        f = self.model.encode_image(images.to(self.model.device))
        return self.adapt_features(ops.l2norm_fwd(f.float().contiguous()), update)

    @torch.no_grad()
    def adapt_view_features(self, feats: torch.Tensor, rho: float = 0.1, update: bool = True) -> TDAResult:
        """``feats`` [G, V, d]: the unit features of V views of each of G images, in stream order.  Per image the
        ``max(1, int(V * rho))`` views of lowest zero-shot entropy are selected (``ops.tpt_objective``'s selection: ties to
        the lower view index), the mean of their features (NOT renormalised: the logits are linear in it) is the image's
        feature, and the G means go through ``adapt_features`` in order.  Never synchronises with the host."""
        if feats.dim() != 3 or feats.shape[2] != self.width or feats.shape[1] < 1:
            raise ValueError(f"adapt_view_features: expected feats [G, V, {self.width}], got {tuple(feats.shape)}")
        if not 0.0 < rho <= 1.0:
            raise ValueError(f"adapt_view_features: rho = {rho} must be in (0, 1]")
        feats = feats.detach().to(device=self.device, dtype=torch.float32).contiguous()
        G, V, d = feats.shape
        K = max(1, int(V * rho))
        _, selected, _, _ = ops.tpt_objective(feats, self.text, K, logit_scale=self.hyper["logit_scale"], want_grad=False)
        picked = torch.gather(feats, 1, selected.long().unsqueeze(-1).expand(G, K, d))
        return self.adapt_features(picked.mean(dim=1), update)

    @torch.no_grad()
    def adapt_views(self, views: torch.Tensor, rho: float = 0.1, update: bool = True) -> TDAResult:
        """``views`` [G, V, 3, R, R] (``clipfs.augmix.view_groups``): one image tower pass over the G V views, one
        normalisation, then ``adapt_view_features``."""
        if self.model is None:
            raise ValueError("adapt_views: the adapter was built without a clip_model")
        if views.dim() != 5:
            raise ValueError(f"adapt_views: expected views [G, V, 3, R, R], got {tuple(views.shape)}")
        G, V = views.shape[:2]
        f = self.model.encode_image(views.to(self.model.device).reshape(G * V, *views.shape[2:]))
        f = ops.l2norm_fwd(f.float().contiguous())
        return self.adapt_view_features(f.view(G, V, -1), rho, update)


@torch.no_grad()
def evaluate_tda(model, loader, adapter: TestTimeDynamicAdapter) -> dict:
    """Streams ``loader`` (batches ``(images, target)`` or a ``clipfs.data`` loader's ``(images, raw, target, index)``)
    through ``adapter`` in order, updating the caches, and returns {"top1_clip": zero-shot accuracy, "top1_tda": accuracy
    of the adapted logits, "n": images}.  The counts stay on the device until the end."""
    if adapter.model is None:
        adapter.model = model
    hits = torch.zeros(2, device=adapter.device, dtype=torch.int64)
    n = 0
    for batch in loader:
        images, target = (batch[0], batch[1]) if len(batch) == 2 else (batch[0], batch[2])
        res = adapter.adapt_images(images)
        target = target.to(adapter.device)
        hits[0] += (res.clip_pred.long() == target).sum()
        hits[1] += (res.logits.argmax(dim=1) == target).sum()
        n += int(target.numel())
    if n == 0:
        raise ValueError("evaluate_tda: the loader yielded no batch")
    h = hits.tolist()
    return {"top1_clip": h[0] / n, "top1_tda": h[1] / n, "n": n}
