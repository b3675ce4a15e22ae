"""Test-time prompt tuning (Shu et al., "Test-Time Prompt Tuning for Zero-Shot Generalization in Vision-Language
Models", NeurIPS 2022) on the HIP engine.  Per test image: the prompt ctx takes ``steps`` (1) AdamW steps that minimise
the entropy of the prediction averaged over the confident augmented views, the tuned ctx classifies the centre view, and
the next image starts from the untouched ctx again.

    select_count          K = max(1, int(V * rho)): the number of confident views
    TestTimePromptTuner   the episodes, a group of G images at a time
    TPTResult             what an ``adapt_*`` call returns

The objective -- view entropies, rank-counting selection, the entropy of the averaged prediction and its gradient with
respect to the class features -- is one ``ops.tpt_objective`` call (csrc/tpt.hip: three launches for the whole group,
deterministic).  The episodes of a group all start from the same ctx, so their first text-tower forward is ONE forward
whose saved activations every episode's backward reads: 2 + 1/G tower passes per image where an episode on its own
pays 3.  The image towers are frozen: ViT and ModifiedResNet towers, with or without frozen LoRA adapters, in every
precision mode.

Not offered: AugMix views (the views are ``tta.make_tta_views``' centre view + random resized crops), training anything
but the ctx, data parallelism, dynamic loss scaling (``loss_scale`` is static), overlapping the next group's image pass
on the side stream, a CoCoOp-style image-conditional ctx.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from clipfs import ops

MAX_VIEWS = 1024  # of clipfs_tpt_objective


def select_count(V: int, rho: float) -> int:
    """The number of confident views kept of ``V``: max(1, int(V * rho))."""
    return max(1, int(V * rho))


class TPTResult(NamedTuple):
    logits: torch.Tensor    # [G, C]  logit_scale * centre view . class features of the tuned ctx
    ctx: torch.Tensor       # [G, n_ctx, d_text]  the tuned ctx of each image
    loss: torch.Tensor      # [G, steps]  the objective before each step
    selected: torch.Tensor  # [G, K] int32  the confident views, ascending view index
    entropy: torch.Tensor   # [G, V]  view entropies under the untouched ctx
    ctx_grad: torch.Tensor  # [G, n_ctx, d_text]  the (unscaled) gradient of the first step


def _trainable_text_side(clip_model):
    """Names of the trainable parameters a text-tower backward would write a gradient for (or silently skip)."""
    text = ("transformer.", "ln_final.", "token_embedding.", "positional_embedding", "text_projection")
    return [n for n, p in clip_model.named_parameters() if p.requires_grad and n.startswith(text)]


class TestTimePromptTuner:
    """Episodes of test-time prompt tuning over ``prompt_learner.ctx`` (a ``slow_pace.VLPromptLearner``: its ``ctx`` and
    ``tokenized_prompts``).  AdamW runs from zero moments with torch's defaults; ``logit_scale`` is a host constant
    (never read from the device).  ``loss_scale`` (a positive float, or None) multiplies the objective's gradient and is
    divided out in the optimiser step: for the fp16 storage mode, whose backward keeps activation gradients as f16.

    An ``adapt_*`` call never synchronises with the host (after the first call on a prompt table, which builds the text
    tower's row plan) and leaves no trace: ``prompt_learner.ctx``, its ``.grad``, the engine's dropout seed counter (seed
    0 throughout: the model's eval behaviour) and every adapter gradient slot are bitwise what they were.

    ValueError for: a trainable text-side adapter, bias or deep prompt (freeze it with ``requires_grad_(False)``: only the
    ctx is tuned), a merged model (``unmerge_lora`` first), ``rho`` outside (0, 1], ``steps`` < 1, a ``loss_scale`` that
    is not a positive float, more than 1024 views.  See the module docstring for what is not offered."""

    __test__ = False  # not a test class, whatever the name says to a collector

    def __init__(self, clip_model, prompt_learner, *, rho: float = 0.1, lr: float = 5e-3, steps: int = 1,
                 betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.01, logit_scale: float = 100.0,
                 loss_scale: Optional[float] = None):
        if not 0.0 < rho <= 1.0:
            raise ValueError(f"TestTimePromptTuner: rho = {rho} must lie in (0, 1] (the share of views kept)")
        if int(steps) != steps or steps < 1:
            raise ValueError(f"TestTimePromptTuner: steps = {steps} must be an integer >= 1")
        if loss_scale is not None and not (isinstance(loss_scale, (int, float)) and 0.0 < loss_scale < float("inf")):
            raise ValueError(f"TestTimePromptTuner: loss_scale = {loss_scale!r} must be a positive float or None "
                             "(only a static scale is offered)")
        self.model, self.learner = clip_model, prompt_learner
        self.rho, self.lr, self.steps = float(rho), float(lr), int(steps)
        self.betas, self.eps, self.wd = (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.logit_scale = float(logit_scale)
        self.loss_scale = None if loss_scale is None else float(loss_scale)
        self._ids = None
        self._refuse()

    def _prompt_ids(self) -> torch.Tensor:
        """The learner's prompt table as the int64 device tensor the engine keys its row plan on: converted once per
        table, so that later calls find the plan and do not synchronise."""
        src = self.learner.tokenized_prompts
        hit = self._ids
        if hit is None or hit[0] is not src or hit[1] != src._version:
            self._ids = hit = (src, src._version, src.to(device=self.model.device, dtype=torch.int64).contiguous())
        return hit[2]

    def _refuse(self) -> None:
        bad = _trainable_text_side(self.model)
        if bad:
            raise ValueError("TestTimePromptTuner tunes the prompt ctx alone, but these text-side parameters are trainable: "
                             f"{', '.join(bad)} -- freeze them with requires_grad_(False)")
        eng = getattr(self.model, "_engine", None)  # no engine is built to answer
        if eng is not None:
            eng.refuse_merged("TestTimePromptTuner")

    @torch.no_grad()
    def adapt_views(self, views: torch.Tensor) -> TPTResult:
        """``views`` [G, V, 3, R, R] (view 0 = the centre view, e.g. G stacked ``tta.make_tta_views``): one no-grad image
        tower pass over the G * V views, one normalisation, then ``adapt_features``."""
        if views.dim() != 5:
            raise ValueError(f"adapt_views: expected views [G, V, 3, R, R], got {tuple(views.shape)}")
        G, V = views.shape[:2]
        self._check_views(V)
        self._refuse()
        flat = views.reshape(G * V, *views.shape[2:]).to(device=self.model.device, dtype=torch.float32)
        feat, _ = self.model.engine.vit_forward(flat, False, 0)
        return self.adapt_features(ops.l2norm_fwd(feat.float().contiguous()).reshape(G, V, -1))

    def _check_views(self, V: int) -> None:
        if not 1 <= V <= MAX_VIEWS:
            raise ValueError(f"TestTimePromptTuner: {V} views per image; the objective kernel takes 1 ... {MAX_VIEWS} "
                             "-- pass fewer views")

    @torch.no_grad()
    def adapt_features(self, feats: torch.Tensor) -> TPTResult:
        """``feats`` [G, V, d]: unit image features of the V views of G images (view 0 = the centre view)."""
        if feats.dim() != 3:
            raise ValueError(f"adapt_features: expected feats [G, V, d], got {tuple(feats.shape)}")
        G, V, _ = feats.shape
        self._check_views(V)
        self._refuse()
        eng = self.model.engine
        eng.refuse_merged("TestTimePromptTuner")
        feats = feats.detach().float().contiguous()
        dev = feats.device
        ids = self._prompt_ids()
        ctx0 = self.learner.ctx.detach()
        K = select_count(V, self.rho)
        s = self.logit_scale
        gscale = 1.0 if self.loss_scale is None else self.loss_scale

        ctx = ctx0.unsqueeze(0).repeat(G, 1, 1).contiguous()  # [G, n_ctx, d_text]: the flat buffer AdamW steps
        grads = torch.zeros_like(ctx)
        m, v = torch.zeros_like(ctx), torch.zeros_like(ctx)
        losses = []
        selected = entropy = ctx_grad = None
        for t in range(1, self.steps + 1):
            if t == 1:  # every episode starts from the same ctx: ONE forward, G backwards off its saved record
                f, rec = eng.text_forward(ids, ctx0, True, 0, own_saved=True)
                T, inv = ops.l2norm_fwd(f, save_inv=True)
                recs, Ts, invs = [rec] * G, [T] * G, [inv] * G
                loss, selected, dT, entropy = ops.tpt_objective(feats, T, K, s, grad_scale=gscale, want_entropy=True)
            else:
                recs, Ts, invs = [], [], []
                Tall = torch.empty(G, T.shape[0], T.shape[1], device=dev, dtype=torch.float32)
                for g in range(G):
                    f, rec = eng.text_forward(ids, ctx[g], True, 0, own_saved=True)
                    _, inv = ops.l2norm_fwd(f, save_inv=True, out=Tall[g])
                    recs.append(rec)
                    Ts.append(Tall[g])
                    invs.append(inv)
                grads.zero_()
                loss, _, dT, _ = ops.tpt_objective(feats, Tall, K, s, selected=selected, grad_scale=gscale)
            losses.append(loss)
            for g in range(G):  # all the backwards before any forward of the stepped ctxs
                eng.text_backward(recs[g], ops.l2norm_bwd(dT[g], Ts[g], invs[g]), grads[g])
            if t == 1:
                ctx_grad = grads * (1.0 / gscale) if self.loss_scale is not None else grads.clone()
            ops.adamw_ext(ctx.view(-1), grads.view(-1), m.view(-1), v.view(-1), t, self.lr, self.betas, self.eps, self.wd,
                          grad_scale=1.0 / gscale)

        logits = []
        for g in range(G):  # the tuned ctxs classify their centre views
            f, _ = eng.text_forward(ids, ctx[g], False, 0)
            logits.append(ops.gemm_nt(feats[g, :1], ops.l2norm_fwd(f), alpha=s))
        return TPTResult(torch.cat(logits), ctx, torch.stack(losses, dim=1), selected, entropy, ctx_grad)
