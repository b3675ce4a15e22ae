"""PLOT (Chen et al., "PLOT: Prompt Learning with Optimal Transport for Vision-Language Models", ICLR 2023) on the HIP
engine: N learnable prompts per class, an image scored by the optimal-transport plan between its M local token features
and the class's N prompt features,

    logits[b, c] = scale * <T, z>,   z = tokens[b] prompts[c]^T,   T = Sinkhorn(exp((z - 1) / eps), iters)

    PLOTPromptLearner   N ctx blocks (views of one flat [N, n_ctx, d] buffer) over the prompts "X X X X name."
    PLOTClassifier      prompt features [C, N, e], logits on cached tokens or on images
    collect_tokens      the frozen image tower's unit local tokens and labels of a pool, cached once
    PLOTTrainer         trains the ctx blocks alone: N text passes, one matching launch, one cross entropy, the matching
                        and text backwards, ONE AdamW launch on the flat buffer per step
    evaluate_plot       top-1 accuracy

The matching (csrc/ot_match.hip, include/clipfs.h "OT matching") keeps the [B, C, M, N] similarity on chip, is
deterministic and holds the plan constant in the backward, as PLOT does.  Stated differences from the paper: the number of
Sinkhorn iterations is fixed (no early stop on the change of u: a data-dependent loop and a host read); the paper trains
with SGD, this trainer with AdamW, the optimiser this library has a kernel for; the marginals are uniform.  Not
offered: ModifiedResNet local features, more than 256 local tokens, gradients through the plan or into the image
tower, data parallelism, loss scaling, EMA.  Accuracy on real checkpoints has not been measured.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from clipfs import engine as E
from clipfs import ops
from slow_pace import PromptBatch


def _refuse_model(clip_model, who: str) -> None:
    """What this method does not train or cannot use, by name."""
    if E._is_resnet(clip_model.visual):
        raise ValueError(f"{who}: a ModifiedResNet image tower has no local tokens here (its attention-pool head computes one "
                         "query row only) -- ViT towers only")
    names = [n for n, p in clip_model.named_parameters() if p.requires_grad]
    if names:
        raise ValueError(f"{who}: the model has trainable adapters, biases or prompts ({names[0]}, {len(names)} in all); PLOT "
                         "trains its own prompt ctx alone -- freeze them (requires_grad_(False))")
    clip_model.engine.refuse_merged(who)


class PLOTPromptLearner(nn.Module):
    """``n_prompts`` independent ctx blocks [n_ctx, d], each drawn from N(0, ctx_std^2) (PLOT's initialisation), as views
    of ONE flat Parameter ``ctx`` [N, n_ctx, d]; the token ids of "X X X X name." are built once.  ``forward()`` returns
    the N PromptBatches of the engine's text route."""

    def __init__(self, classnames: Sequence[str], clip_model, n_prompts: int = 4, n_ctx: int = 4, ctx_std: float = 0.02,
                 seed: int = 0, token_ids: Optional[torch.Tensor] = None):
        super().__init__()
        if not 1 <= n_prompts <= 32:
            raise ValueError(f"PLOTPromptLearner: n_prompts = {n_prompts} outside [1, 32]")
        if n_ctx < 1:
            raise ValueError(f"PLOTPromptLearner: n_ctx = {n_ctx}")
        if token_ids is None:
            from jclip import clip
            names = [name.replace("_", " ") for name in classnames]
            token_ids = clip.tokenize([" ".join(["X"] * n_ctx) + " " + name + "." for name in names])
        if token_ids.dim() != 2 or token_ids.shape[1] != clip_model.context_length:
            raise ValueError(f"PLOTPromptLearner: token ids {tuple(token_ids.shape)}, expected [C, {clip_model.context_length}]")
        d = clip_model.token_embedding.weight.shape[1]
        g = torch.Generator().manual_seed(seed)
        ctx = torch.randn(n_prompts, n_ctx, d, generator=g, dtype=torch.float32) * ctx_std
        self.ctx = nn.Parameter(ctx.to(clip_model.device).contiguous())
        self.tokenized_prompts = token_ids.to(clip_model.device)
        self.n_cls, self.n_ctx, self.n_prompts = token_ids.shape[0], n_ctx, n_prompts
        self._model = [clip_model]  # not registered as a sub-module

    @classmethod
    def from_token_ids(cls, token_ids: torch.Tensor, clip_model, **kw) -> "PLOTPromptLearner":
        """Prompts already tokenised ([C, context_length]; the ctx blocks replace positions 1 .. n_ctx)."""
        return cls((), clip_model, token_ids=token_ids, **kw)

    def block(self, n: int) -> torch.Tensor:
        """ctx block n: a [n_ctx, d] view of the flat buffer (differentiable: its gradient lands in ``ctx.grad[n]``)."""
        return self.ctx[n]

    def forward(self) -> List[PromptBatch]:
        return [PromptBatch(self.ctx[n], self.tokenized_prompts) for n in range(self.n_prompts)]


class PLOTClassifier(nn.Module):
    """Scores local tokens against the learner's prompts.  ``eps`` in [0.05, 10] and ``iters`` in [1, 1000] are the
    matching's; the logit scale is the model's ``logit_scale.exp()``, read once."""

    def __init__(self, clip_model, learner: PLOTPromptLearner, eps: float = 0.1, iters: int = 100):
        super().__init__()
        _refuse_model(clip_model, "PLOTClassifier")
        self.learner = learner
        self.eps, self.iters = float(eps), int(iters)
        self.scale = float(clip_model.logit_scale.detach().exp().item())
        self._model = [clip_model]

    @property
    def model(self):
        return self._model[0]

    def text_features(self) -> torch.Tensor:
        """[C, N, e] unit rows: N passes of the differentiable ``encode_text`` over the same token ids, one per ctx block."""
        lr = self.learner
        feats = [E.l2_normalize(E.encode_text(self.model, lr.tokenized_prompts, lr.block(n))) for n in range(lr.n_prompts)]
        return torch.stack(feats, dim=1)

    def logits(self, tokens: torch.Tensor, text: Optional[torch.Tensor] = None) -> torch.Tensor:
        """logits [B, C] of unit local tokens [B, M, e] (never normalised here); differentiable w.r.t. the ctx blocks."""
        text = self.text_features() if text is None else text
        return ops.ot_match(tokens.float(), text.contiguous(), None, None, self.eps, self.iters, self.scale)

    def tokens(self, images: torch.Tensor) -> torch.Tensor:
        """Unit local tokens [B, P, e] of ``images`` (no graph: the image tower is frozen)."""
        t = E.encode_image_tokens(self.model, images)
        return ops.l2norm_fwd(t.view(-1, t.shape[2])).view_as(t)

    def forward(self, images: torch.Tensor) -> torch.Tensor:
        return self.logits(self.tokens(images))


@torch.no_grad()
def collect_tokens(clip_model, loader, epochs: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """(tokens [N, P, e] unit rows, labels [N] int64) of the loader's pool, row i = pool image i, as
    ``tip_adapter.collect_features`` does for the global feature: each image's unit local tokens summed over ``epochs``
    augmentation passes, divided by ``epochs`` and renormalised.  Each index occurs once per epoch (``drop_last`` must be
    off), so the result is deterministic whatever the shuffle."""
    if epochs < 1:
        raise ValueError(f"collect_tokens: epochs = {epochs}")
    if getattr(loader, "drop_last", False):
        raise ValueError("collect_tokens: the loader drops the last batch, so some pool images would get no tokens")
    n = len(loader.pool)
    acc = None
    for _ in range(epochs):
        for images, _raw, _target, index in loader:
            if images is None:
                raise ValueError("collect_tokens: the loader must yield the 'clip' output")
            t = E.encode_image_tokens(clip_model, images)
            t = ops.l2norm_fwd(t.view(-1, t.shape[2])).view_as(t)
            if acc is None:
                acc = torch.zeros(n, t.shape[1], t.shape[2], device=t.device, dtype=torch.float32)
            acc.index_copy_(0, index, acc.index_select(0, index) + t)  # unique indices: one writer per row
    if acc is None:
        raise ValueError("collect_tokens: the loader yielded no batch")
    acc.mul_(1.0 / epochs)
    return ops.l2norm_fwd(acc.view(-1, acc.shape[2])).view_as(acc), loader.pool.labels.clone()


class PLOTTrainer:
    """AdamW on the ctx blocks alone.  The blocks, their gradient and both moments live in flat fp32 buffers
    (``learner.ctx`` becomes a view of the first).  A step is N text-tower passes (one per block, each keeping its own
    activations), the normalisations, ONE matching launch, the one cross-entropy kernel, the matching's dP launch, N text
    backwards that write block n's gradient into its slice of the flat gradient, and ONE ``ops.adamw`` launch at the
    pre-step learning rate; then the cosine schedule (with ``T_max``) advances.  ``step`` never synchronises with the host.
    The paper trains with SGD; AdamW is the optimiser this library has a kernel for."""

    def __init__(self, classifier: PLOTClassifier, lr: float = 2e-3, weight_decay: float = 5e-4, betas=(0.9, 0.999),
                 eps: float = 1e-8, T_max: Optional[int] = None):
        model, learner = classifier.model, classifier.learner
        _refuse_model(model, "PLOTTrainer")
        if not learner.ctx.is_cuda:
            raise ValueError("PLOTTrainer: the learner must be on the GPU (there is no CPU path)")
        self.classifier = classifier
        self.params = learner.ctx.detach().clone().contiguous().view(-1)
        learner.ctx.data = self.params.view_as(learner.ctx)
        self.grads = torch.zeros_like(self.params)
        self.m = torch.zeros_like(self.params)
        self.v = torch.zeros_like(self.params)
        self.lr, self.wd, self.betas, self.eps = float(lr), float(weight_decay), tuple(betas), float(eps)
        self.t = 0
        self.sched = None
        if T_max is not None:
            from slow_pace import CosineAnnealingLR
            self.sched = CosineAnnealingLR(self.lr, T_max)

    @property
    def ctx_grad(self) -> torch.Tensor:
        """The gradient of the last step's mean cross entropy, [N, n_ctx, d] (a view of the flat buffer)."""
        return self.grads.view_as(self.classifier.learner.ctx)

    @torch.no_grad()
    def step(self, tokens: torch.Tensor, labels: torch.Tensor):
        """One optimiser step on cached unit ``tokens`` [B, M, e] with ``labels`` [B] int64: returns (loss [1] fp32, the
        batch's mean cross entropy, and correct [1] int32), device tensors."""
        cl = self.classifier
        model, learner = cl.model, cl.learner
        eng = model.engine
        eng.refuse_merged("PLOTTrainer.step")
        x = tokens.detach().float().contiguous()
        B = x.shape[0]
        N, C = learner.n_prompts, learner.n_cls
        ctx = self.params.view_as(learner.ctx)
        gctx = self.grads.view_as(learner.ctx)
        passes = []
        text = None
        for n in range(N):
            feat, c = eng.text_forward(learner.tokenized_prompts, ctx[n], True, eng.next_seed() if model.training else 0,
                                       own_saved=True)
            y, inv = ops.l2norm_fwd(feat, save_inv=True)
            if text is None:
                text = torch.empty(C, N, y.shape[1], device=y.device, dtype=torch.float32)
            text[:, n].copy_(y)
            passes.append((c, y, inv))
        logits, u, v = ops.ot_logits(x, text, None, None, cl.eps, cl.iters, cl.scale)
        loss_sum, dlogits, correct = ops.cross_entropy(logits, labels.to(x.device).long().contiguous())
        dtext, _ = ops.ot_bwd(x, text, u, v, dlogits, cl.eps, cl.scale)
        self.grads.zero_()
        for n, (c, y, inv) in enumerate(passes):
            eng.text_backward(c, ops.l2norm_bwd(dtext[:, n].contiguous(), y, inv), gctx[n])
        self.t += 1
        ops.adamw(self.params, self.grads, self.m, self.v, self.t, self.lr, self.betas, self.eps, self.wd)
        if self.sched is not None:
            self.lr = self.sched.step()
        return loss_sum * (1.0 / B), correct

    def state_dict(self) -> dict:
        """Everything a bit-for-bit resume needs (tensors are clones)."""
        s = self.sched
        return {"params": self.params.clone(), "m": self.m.clone(), "v": self.v.clone(), "t": int(self.t), "lr": float(self.lr),
                "hyper": {"weight_decay": self.wd, "betas": tuple(self.betas), "eps": self.eps},
                "match": {"eps": self.classifier.eps, "iters": self.classifier.iters, "scale": self.classifier.scale},
                "scheduler": None if s is None else {"base_lr": s.base_lr, "T_max": s.T_max, "eta_min": s.eta_min,
                                                     "last_epoch": s.last_epoch}}

    def load_state_dict(self, sd: dict) -> None:
        if sd["params"].numel() != self.params.numel():
            raise ValueError(f"the saved state holds {sd['params'].numel()} ctx elements, this learner {self.params.numel()}")
        if (self.sched is None) != (sd["scheduler"] is None):
            raise ValueError("the saved state " + ("has no" if self.sched is not None else "carries a")
                             + " scheduler position: the trainer was built with another T_max setting")
        for dst, key in ((self.params, "params"), (self.m, "m"), (self.v, "v")):
            dst.copy_(sd[key])
        self.t, self.lr = int(sd["t"]), float(sd["lr"])
        h, mt = sd["hyper"], sd["match"]
        self.wd, self.betas, self.eps = float(h["weight_decay"]), tuple(h["betas"]), float(h["eps"])
        self.classifier.eps, self.classifier.iters, self.classifier.scale = float(mt["eps"]), int(mt["iters"]), float(mt["scale"])
        if self.sched is not None:
            s = sd["scheduler"]
            self.sched.base_lr, self.sched.T_max = float(s["base_lr"]), int(s["T_max"])
            self.sched.eta_min, self.sched.last_epoch = float(s["eta_min"]), int(s["last_epoch"])


@torch.no_grad()
def evaluate_plot(classifier: PLOTClassifier, tokens: torch.Tensor, labels: torch.Tensor, batch: int = 256) -> float:
    """Top-1 accuracy of the classifier on cached unit ``tokens`` [N, M, e] with ``labels`` [N]; the prompt features are
    computed once.  Ties go to the lower class index."""
    text = classifier.text_features().detach()
    labels = labels.to(tokens.device).long()
    hits = torch.zeros((), device=tokens.device, dtype=torch.int64)
    for lo in range(0, tokens.shape[0], batch):
        logits = classifier.logits(tokens[lo:lo + batch].contiguous(), text)
        hits += (logits.argmax(1) == labels[lo:lo + batch]).sum()
    return float(hits.item()) / max(1, tokens.shape[0])
