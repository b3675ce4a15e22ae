"""Transductive zero-/few-shot inference (TransCLIP: Zanella, Gerin and Ben Ayed, "Boosting Vision-Language Models with
Transduction", NeurIPS 2024) on the HIP engine: the whole unlabelled test set is classified at once.  Every test feature
is tied to its k nearest neighbours among the test features, every class gets a Gaussian (its mean, one shared diagonal
variance), and the assignments z, the means and the variance are updated in turn, anchored to the zero-shot
log-probabilities (and to labelled shots when there are some).  No labels, no backward pass, no tower pass beyond the
features; it stacks on any classifier that yields class features: zero-shot text features, prompt-tuned class features,
a LoRA-tuned model's features.

    TransductiveClassifier   class features and hyper-parameters; ``fit_predict`` / ``fit_predict_images``
    TransductiveResult       what a fit returns
    evaluate_transductive    top-1 accuracy of a loader before and after the transduction

The rule is written out in include/clipfs.h ("TRANSDUCT").  ``ops.transduct_fit`` (csrc/transduct.hip) runs it in 6 + (kNN
chunks > 1) + outer (inner + 4) launches whatever the shapes, without a host synchronisation, bitwise equal run to run;
the N x N similarities of the kNN affinity never reach memory.

Not offered: features spread over data-parallel ranks (one rank holds the set), fp16 / bf16 storage of z, a symmetrised or
thresholded affinity, a support-to-query affinity, early stopping on convergence (it would need the host), hyper-parameter
search.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from clipfs import ops

MAX_ROWS = 131072  # of clipfs_transduct_fit


class TransductiveResult(NamedTuple):
    z: torch.Tensor                 # [N, C]  the assignments (rows sum to one)
    labels: torch.Tensor            # [N] int32  argmax z, ties to the lower class
    zero_shot_labels: torch.Tensor  # [N] int32  argmax of the zero-shot logits, ties to the lower class
    mu: torch.Tensor                # [C, d]  the class means
    var: torch.Tensor               # [d]  the shared diagonal variance
    neighbours: torch.Tensor        # [N, k] int32  per row its k most similar other rows, descending
    weights: torch.Tensor           # [N, k]  their similarities


class TransductiveClassifier:
    """Class features: ``text_features`` [C, d] (normalised here), or ``clip_model`` plus ``class_features`` [C, d] /
    ``tokenized_prompts`` [C, L] (encoded once with ``encode_text``); ``clip_model`` is also what ``fit_predict_images``
    runs.  Hyper-parameters are those of ``ops.TRANSDUCT_DEFAULTS`` (logit_scale 100, k 3, init_top 8, lam 1, shot_weight 1,
    outer 10, inner 5, n_min 1e-6, var_floor 1e-6).

    ValueError for an unknown hyper-parameter, k outside [1, 8], init_top outside [1, 16], outer or inner below 1, class
    features that are not [n_classes, d]."""

    def __init__(self, text_features: Optional[torch.Tensor] = None, *, clip_model=None, class_features=None,
                 tokenized_prompts=None, n_classes: Optional[int] = None, device=None, **hyper):
        unknown = sorted(set(hyper) - set(ops.TRANSDUCT_DEFAULTS))
        if unknown:
            raise ValueError(f"TransductiveClassifier: unknown hyper-parameter(s) {', '.join(unknown)}; known: "
                             f"{', '.join(sorted(ops.TRANSDUCT_DEFAULTS))}")
        self.hyper = {**ops.TRANSDUCT_DEFAULTS, **hyper}
        for name, lo, hi in (("k", 1, 8), ("init_top", 1, 16), ("outer", 1, None), ("inner", 1, None)):
            v = self.hyper[name]
            if int(v) != v or v < lo or (hi is not None and v > hi):
                raise ValueError(f"TransductiveClassifier: {name} = {v} must be an integer in [{lo}, {hi if hi else 'inf'}]")
            self.hyper[name] = int(v)
        self.model = clip_model
        feats = text_features if text_features is not None else class_features
        if feats is None:
            if clip_model is None or tokenized_prompts is None:
                raise ValueError("TransductiveClassifier: give text_features, or clip_model with class_features or "
                                 "tokenized_prompts")
            with torch.no_grad():
                feats = clip_model.encode_text(tokenized_prompts.to(clip_model.device))
        if device is None:
            device = clip_model.device if clip_model is not None else feats.device
        feats = feats.detach().to(device=device, dtype=torch.float32).contiguous()
        if feats.dim() != 2 or (n_classes is not None and feats.shape[0] != n_classes):
            raise ValueError(f"TransductiveClassifier: class features {tuple(feats.shape)} are not [n_classes = {n_classes}, d]")
        self.text = ops.l2norm_fwd(feats)
        self.n_classes, self.width = self.text.shape
        self.device = self.text.device

    @torch.no_grad()
    def fit_predict(self, features: torch.Tensor, support_features: Optional[torch.Tensor] = None,
                    support_labels: Optional[torch.Tensor] = None) -> TransductiveResult:
        """``features`` [N, d] unit test features, N in [max(k + 1, init_top), 131072]; optionally labelled shots
        ``support_features`` [M, d] (unit rows) with ``support_labels`` [M].  Labels given as a CPU tensor are checked for
        range before anything is enqueued; a device tensor is used as it is.  Never synchronises with the host."""
        if features.dim() != 2 or features.shape[1] != self.width:
            raise ValueError(f"fit_predict: expected features [N, {self.width}], got {tuple(features.shape)}")
        n_lo = max(self.hyper["k"] + 1, self.hyper["init_top"])
        if not n_lo <= features.shape[0] <= MAX_ROWS:
            raise ValueError(f"fit_predict: N = {features.shape[0]} outside [{n_lo}, {MAX_ROWS}]")
        if (support_features is None) != (support_labels is None):
            raise ValueError("fit_predict: support_features and support_labels come together")
        feats = features.detach().to(device=self.device, dtype=torch.float32).contiguous()
        if support_features is not None:
            if support_features.dim() != 2 or support_features.shape[1] != self.width or \
                    support_labels.numel() != support_features.shape[0]:
                raise ValueError(f"fit_predict: expected support_features [M, {self.width}] and support_labels [M]")
            support_features = support_features.detach().to(device=self.device, dtype=torch.float32).contiguous()
        out = ops.transduct_fit(feats, self.text, support_features, support_labels, **self.hyper)
        return TransductiveResult(out["z"], out["labels"], out["zs_labels"], out["mu"], out["var"], out["nbr"], out["w"])

    @torch.no_grad()
    def fit_predict_images(self, images: torch.Tensor) -> TransductiveResult:
        """Image tower forward (ViT or ModifiedResNet, any precision mode), normalisation, then ``fit_predict``."""
        if self.model is None:
            raise ValueError("fit_predict_images: the classifier was built without a clip_model")
        f = self.model.encode_image(images.to(self.model.device))
        return self.fit_predict(ops.l2norm_fwd(f.float().contiguous()))


@torch.no_grad()
def evaluate_transductive(model, loader, classifier: TransductiveClassifier, support=None) -> dict:
    """Encodes every batch of ``loader`` (batches ``(images, target)`` or a ``clipfs.data`` loader's ``(images, raw, target,
    index)``) with ``model.encode_image``, fits the whole set at once and returns {"top1_zero_shot", "top1_transductive",
    "moved": labels the transduction changed, "n"}.  ``support``: (features [M, d], labels [M]) of labelled shots."""
    feats, targets = [], []
    for batch in loader:
        images, target = (batch[0], batch[1]) if len(batch) == 2 else (batch[0], batch[2])
        f = model.encode_image(images.to(model.device))
        feats.append(ops.l2norm_fwd(f.float().contiguous()))
        targets.append(target.to(classifier.device))
    if not feats:
        raise ValueError("evaluate_transductive: the loader yielded no batch")
    target = torch.cat(targets)
    res = classifier.fit_predict(torch.cat(feats), *(support if support is not None else ()))
    n = int(target.numel())
    hits = torch.stack([(res.zero_shot_labels.long() == target).sum(), (res.labels.long() == target).sum(),
                        (res.labels != res.zero_shot_labels).sum()]).tolist()
    return {"top1_zero_shot": hits[0] / n, "top1_transductive": hits[1] / n, "moved": hits[2], "n": n}
