"""Times test-time prompt tuning (tpt.py, csrc/tpt.hip) against the composed route built from what the tree had before it.

(a) the objective alone -- view entropies, confident-view selection, the entropy of the averaged prediction and its
    gradient with respect to the class features, for G = 8 images of 64 views:
        fused     ops.tpt_objective (3 launches)
        composed  ops.gemm_nt for the logits, torch log_softmax / topk / gather / logsumexp under autograd, ops.gemm_nt
                  per image for the class-feature gradient
    at (C 403, d 512) and (C 1000, d 1024), with the number of kernels each side launches (torch.profiler).
(b) whole episodes on ViT-B/32 geometry with synthetic weights, 403 prompts, 64 views of 224 x 224, G = 1 and 8 images per
    call, views in, logits out:
        fused     TestTimePromptTuner.adapt_views
        composed  the same image pass, then per image: slow_pace.TextEncoder on the autograd route, torch ops for the
                  objective, torch.optim.AdamW, a second no-grad text pass, the centre view's logits
        mta       ood.score_views on the same views (training-free; for scale)
    and the episodes alone on precomputed features (adapt_features against the composed loop), which leaves out the image
    pass both sides share.

The arms alternate call by call in one process, warm; each call is timed with a pair of events on the stream and the
medians over ``--calls`` calls (at least 20) are reported.

    python scripts/bench_tpt.py [--calls 20] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "jittor-clip-fewshot_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

S = 100.0


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(arms, calls):
    """{name: (median, min, max) ms} of the callables in ``arms`` called in turn, ``calls`` rounds, after two warm rounds."""
    for _ in range(2):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for _ in range(calls):
        for k, fn in arms.items():
            t[k].append(_time(fn))
    return {k: {"ms": round(statistics.median(v), 4), "min_max_ms": [round(min(v), 4), round(max(v), 4)], "calls": len(v)}
            for k, v in t.items()}


def count_kernels(fn):
    """Kernels ``fn`` launches (copies and memsets left out), or the reason they could not be counted."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA")]
        return sum(1 for n in names if not any(w in n.lower() for w in ("memcpy", "memset", "copybuffer", "fillbuffer")))
    except Exception as e:  # a profiler that is not usable here is reported, not hidden
        return f"not counted: {type(e).__name__}: {e}"


class _Logits(torch.autograd.Function):
    """z [V, C] = s F T^T of one image with ops.gemm_nt, differentiable with respect to T."""

    @staticmethod
    def forward(ctx, feats, T):
        from clipfs import ops
        ctx.save_for_backward(feats)
        return ops.gemm_nt(feats, T, alpha=S)

    @staticmethod
    def backward(ctx, dz):
        from clipfs import ops
        (feats,) = ctx.saved_tensors
        return None, ops.gemm_nt(dz.t().contiguous(), feats.t().contiguous(), alpha=S)


def composed_loss(z, K):
    """The released method's objective from logits z [G, V, C] with torch ops: loss [G]."""
    lp = torch.log_softmax(z, dim=-1)
    H = -(lp.exp() * lp).sum(-1)
    idx = torch.topk(H, K, dim=1, largest=False).indices
    sel = lp.gather(1, idx[..., None].expand(-1, -1, lp.shape[-1]))
    avg = torch.logsumexp(sel, dim=1) - math.log(K)
    return -(avg.exp() * avg).sum(-1)


def _inputs(V, C, d, seed):
    """Unit view features [V, d] that lean towards one class each by a varying amount, and unit class features [C, d]
    around a common mean: entropies from ~0.01 to ~log C at a logit scale of 100 (plain random unit vectors saturate)."""
    g = torch.Generator().manual_seed(seed)
    unit = lambda t: t / t.norm(dim=-1, keepdim=True)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    m, R = unit(r(d)), unit(r(C, d))
    T = unit(m + 0.5 * R)
    cls = torch.randint(C, (V,), generator=g)
    a = torch.linspace(0.05, 0.45, V, dtype=torch.float64)[torch.randperm(V, generator=g)]
    F = unit(m + 0.5 * (a[:, None] * R[cls] + (1 - a * a).sqrt()[:, None] * unit(r(V, d))))
    return F.float(), T.float()


def bench_objective(G, V, C, d, calls, dev):
    from clipfs import ops
    pairs = [_inputs(V, C, d, s) for s in range(G)]
    feats = torch.stack([p[0] for p in pairs]).to(dev)
    T = pairs[0][1].to(dev)
    K = max(1, int(V * 0.1))
    Texp = T[None].expand(G, -1, -1)

    def fused():
        return ops.tpt_objective(feats, T, K, S)

    def composed():
        Tg = Texp.detach().clone().requires_grad_()  # a leaf per image, as the episodes need the gradients apart
        with torch.enable_grad():
            z = torch.stack([_Logits.apply(feats[g], Tg[g]) for g in range(G)])
            loss = composed_loss(z, K)
            loss.sum().backward()
        return loss, Tg.grad

    lf, _, df, _ = fused()
    lc, dc = composed()
    res = {"shape": dict(G=G, V=V, C=C, d=d, K=K),
           "loss_max_abs_diff_vs_composed": float((lf - lc).abs().max()),
           "dtext_max_abs_diff_vs_composed": float((df - dc).abs().max()), "dtext_max_abs": float(df.abs().max())}
    res.update(alternate({"fused": fused, "composed": composed}, calls))
    res["composed_over_fused"] = round(res["composed"]["ms"] / res["fused"]["ms"], 2)
    res["kernels"] = {"fused": count_kernels(fused), "composed": count_kernels(composed)}
    return res


def build_b32(dev, C=403):
    import slow_pace as SP
    from clipfs import synth
    from jclip.model import build_model
    cfg = synth.VIT_B32
    model = build_model(synth.synth_state_dict(cfg, seed=11, perturb=True), device=dev)
    model.eval()
    ids = synth.synth_captions(C, cfg.context_length, cfg.vocab_size, seed=4, min_len=5, max_len=12).to(dev)
    learner = SP.VLPromptLearner.__new__(SP.VLPromptLearner)
    torch.nn.Module.__init__(learner)
    learner.ctx = torch.nn.Parameter(model.token_embedding.weight.data[ids[0, 1:5]].clone())
    learner.tokenized_prompts, learner.n_ctx, learner.n_cls = ids, 4, C
    learner._model = [model]
    return cfg, model, learner, SP


def bench_episodes(calls, dev):
    import ood
    from clipfs import engine as E
    from clipfs import ops, synth
    from tpt import TestTimePromptTuner, select_count
    cfg, model, learner, SP = build_b32(dev)
    V = 64
    K = select_count(V, 0.1)
    tuner = TestTimePromptTuner(model, learner)
    enc = SP.TextEncoder(model)
    ids = learner.tokenized_prompts
    with torch.no_grad():
        text0 = ops.l2norm_fwd(model.engine.text_forward(ids, learner.ctx.detach(), False, 0)[0])
    out = {"model": cfg.name, "prompts": int(ids.shape[0]), "views": V, "K": K}

    def image_pass(views):
        G = views.shape[0]
        f, _ = model.engine.vit_forward(views.reshape(G * V, *views.shape[2:]), False, 0)
        return ops.l2norm_fwd(f).reshape(G, V, -1)

    def composed_episodes(feats):
        logits = []
        for g in range(feats.shape[0]):
            ctx = torch.nn.Parameter(learner.ctx.detach().clone())
            opt = torch.optim.AdamW([ctx], lr=5e-3)
            with torch.enable_grad():
                T = E.l2_normalize(enc(SP.PromptBatch(ctx, ids)))
                z = S * feats[g] @ T.t()
                composed_loss(z[None], K).sum().backward()
            opt.step()
            with torch.no_grad():
                T2 = ops.l2norm_fwd(enc(SP.PromptBatch(ctx.detach(), ids)))
                logits.append(S * feats[g, :1] @ T2.t())
        return torch.cat(logits)

    for G in (1, 8):
        views = synth.synth_images(G * V, cfg.image_resolution, seed=3).reshape(G, V, 3, cfg.image_resolution,
                                                                                cfg.image_resolution).to(dev)
        with torch.no_grad():
            feats = image_pass(views)
        lf = tuner.adapt_features(feats).logits
        lc = composed_episodes(feats)
        r = {"final_logits_max_abs_diff_vs_composed": float((lf - lc).abs().max())}
        r["views_in"] = alternate({"fused": lambda: tuner.adapt_views(views),
                                   "composed": lambda: composed_episodes(image_pass(views)),
                                   "mta": lambda: ood.score_views(model, views, text0),
                                   "image_pass": lambda: image_pass(views)}, calls)
        r["features_in"] = alternate({"fused": lambda: tuner.adapt_features(feats),
                                      "composed": lambda: composed_episodes(feats)}, calls)
        for k in ("views_in", "features_in"):
            t = r[k]
            t["composed_over_fused"] = round(t["composed"]["ms"] / t["fused"]["ms"], 2)
            for arm in t:
                if isinstance(t[arm], dict):
                    t[arm]["episodes_per_s"] = round(1000.0 * G / t[arm]["ms"], 2)
        out[f"G{G}"] = r
        print(json.dumps({f"episodes_G{G}": r}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    calls = max(20, args.calls)
    out = {"device": torch.cuda.get_device_name(0), "calls": calls}

    def save():
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(out, fh, indent=1)

    out["objective"] = {}
    for name, (C, d) in {"C403_d512": (403, 512), "C1000_d1024": (1000, 1024)}.items():
        out["objective"][name] = bench_objective(8, 64, C, d, calls, dev)
        print(json.dumps({name: out["objective"][name]}), flush=True)
        save()
    out["episodes"] = bench_episodes(calls, dev)
    save()


if __name__ == "__main__":
    main()
