"""Times the contrastive objective (csrc/contrastive.hip) against the route composed from what the tree had before it.

(a) the symmetric loss and both feature gradients of R queries x N keys, both directions:
        fused     two calls of ops.contrastive_objective (the second accumulates into the first one's gradients)
        composed  ops.gemm_nt for the [R, N] logits, torch for the target matrix and the two soft-target softmax cross
                  entropies (one on the transpose) and their logits gradients, four ops.matmul_small for the feature
                  gradients
    at (R, N, d) = (256, 256, 512), (256, 403, 512), (512, 4096, 512), (256, 2048, 1024), with the number of kernels each
    side launches (torch.profiler) and the largest difference between the two routes' results.
(b) one training step at the cfg-2 geometry (ViT-B/32, rank-4 LoRA on q, k, v of all 12 + 12 blocks, 4 prompt tokens, 256
    images): LoRATrainer.step_pairs on 256 captions (pairs) against LoRATrainer.step on the same 256 captions as a class
    table.

The arms alternate call by call in one process, warm; each call is timed with a pair of events on the stream and the
medians over ``--calls`` calls are reported whatever they are.

    python scripts/bench_contrastive.py [--calls 20] [--skip-step] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "jittor-clip-fewshot_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

S = 100.0
SHAPES = [(256, 256, 512), (256, 403, 512), (512, 4096, 512), (256, 2048, 1024)]


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(arms, calls):
    """{name: median, min, max ms} of the callables in ``arms`` called in turn, ``calls`` rounds, after two warm rounds."""
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


def _inputs(R, N, d, seed, dev):
    """Unit rows, groups from min(R, N) // 4 ids with a tenth of each side masked, queries pulled 0.2 towards the mean of
    their positives (the recipe of tests/contrastive_ref.py)."""
    g = torch.Generator().manual_seed(seed)
    unit = lambda t: t / t.norm(dim=-1, keepdim=True)
    q = unit(torch.randn(R, d, generator=g, dtype=torch.float64))
    k = unit(torch.randn(N, d, generator=g, dtype=torch.float64))
    ids = max(2, min(R, N) // 4)
    qg, kg = torch.randint(ids, (R,), generator=g).int(), torch.randint(ids, (N,), generator=g).int()
    qg[torch.randperm(R, generator=g)[:R // 10]] = -1
    kg[torch.randperm(N, generator=g)[:N // 10]] = -1
    pos = ((qg[:, None] == kg[None, :]) & (kg[None, :] >= 0)).double()
    mean = pos @ k
    has = pos.sum(1) > 0
    mean[has] = unit(mean[has])
    q = unit(q + 0.2 * mean)
    return q.float().to(dev), k.float().to(dev), qg.to(dev), kg.to(dev)


def fused(q, k, qg, kg):
    from clipfs import ops
    R, N = q.shape[0], k.shape[0]
    l1, _, _, dq, dk = ops.contrastive_objective(q, k, qg, kg, S, 0.5 / R)
    l2, _, _, dk, dq = ops.contrastive_objective(k, q, kg, qg, S, 0.5 / N, dq=dk, dk=dq)
    return l1 + l2, dq, dk


def composed(q, k, qg, kg):
    from clipfs import ops
    R, d = q.shape
    N = k.shape[0]
    z = ops.gemm_nt(q, k, alpha=S)
    pos = (qg[:, None] == kg[None, :]) & (kg[None, :] >= 0) & (qg[:, None] >= 0)
    posf = pos.float()

    def direction(zz, tt, rows_alive_mask):
        n = tt.sum(1, keepdim=True)
        alive = (n > 0) & rows_alive_mask[:, None]
        lp = torch.log_softmax(zz, dim=1)
        lp = torch.where(torch.isfinite(lp), lp, torch.zeros_like(lp))
        t = tt / n.clamp(min=1)
        rows = -(t * lp).sum(1, keepdim=True)
        w = 0.5 / zz.shape[0]
        G = torch.where(alive, w * (torch.softmax(zz, dim=1) - t), torch.zeros_like(zz))
        return w * rows[alive].sum(), torch.nan_to_num(G)

    # one direction's masked keys are the other's masked queries: columns out of the softmax, rows dropped
    l1, G1 = direction(z.masked_fill(~(kg >= 0)[None, :], float("-inf")), posf, qg >= 0)
    l2, G2 = direction(z.t().masked_fill(~(qg >= 0)[None, :], float("-inf")), posf.t().contiguous(), kg >= 0)
    G1, G2 = G1.contiguous(), G2.contiguous()
    dq = ops.matmul_small(G1, k, R, d, N, N, 1, d, 1, S)
    dk = ops.matmul_small(G1, q, N, d, R, 1, N, d, 1, S)
    dk2 = ops.matmul_small(G2, q, N, d, R, R, 1, d, 1, S)
    dq2 = ops.matmul_small(G2, k, R, d, N, 1, R, d, 1, S)
    return l1 + l2, dq + dq2, dk + dk2


def bench_objective(R, N, d, calls, dev):
    q, k, qg, kg = _inputs(R, N, d, 1, dev)
    a, b = fused(q, k, qg, kg), composed(q, k, qg, kg)
    diff = {"loss": abs(a[0].item() - b[0].item()),
            "dq_share": ((a[1] - b[1]).abs().max() / b[1].abs().max()).item(),
            "dk_share": ((a[2] - b[2]).abs().max() / b[2].abs().max()).item()}
    arms = {"fused": lambda: fused(q, k, qg, kg), "composed": lambda: composed(q, k, qg, kg)}
    t = alternate(arms, calls)
    out = {"R": R, "N": N, "d": d, "fused": t["fused"], "composed": t["composed"],
           "speedup": round(t["composed"]["ms"] / t["fused"]["ms"], 3),
           "kernels": {kname: count_kernels(fn) for kname, fn in arms.items()},
           "logits_and_gradient_bytes_not_materialised": 2 * R * N * 4, "fused_minus_composed": diff}
    print(f"[bench_contrastive] objective {R} x {N} x {d}: fused {t['fused']['ms']} ms, composed {t['composed']['ms']} ms, "
          f"kernels {out['kernels']}", file=sys.stderr)
    return out


def bench_step(calls, dev):
    import lora_train_vlp as L
    from clipfs import synth
    from jclip.model import build_model
    cfg = synth.VIT_B32
    model = build_model(synth.synth_state_dict(cfg, seed=1234), device=dev)
    largs = types.SimpleNamespace(encoder="both", position="all", backbone="ViT-B/32", params=["q", "k", "v"], r=4, alpha=1,
                                  dropout_rate=0.25)
    layers = L.apply_lora(largs, model)
    import contextlib
    with contextlib.redirect_stdout(sys.stderr):
        L.load_lora(largs, layers, os.path.join(ROOT, "tests", "golden", "lora_weights.pkl"))
    L.mark_only_lora_as_trainable(model)
    ids = torch.tensor([320, 1125, 539, 320], device=dev)
    ctx = torch.nn.Parameter(model.token_embedding.weight.data[ids].clone())
    model.train()
    tr = L.LoRATrainer(model, prompt_ctx=ctx)
    B = M = 256
    img = synth.synth_images(B, 224, seed=0).to(dev)
    cap = synth.synth_captions(M, 77, cfg.vocab_size, seed=1).to(dev)
    tgt = synth.synth_labels(B, M, seed=2).to(dev)
    arms = {"step_pairs": lambda: tr.step_pairs(img, cap), "step": lambda: tr.step(img, cap, tgt)}
    t = alternate(arms, calls)
    out = {"geometry": "cfg-2: ViT-B/32, rank-4 LoRA q,k,v on 12 + 12 blocks, 4 prompt tokens, dropout 0.25, 256 images, "
                       "256 captions", "step_pairs": t["step_pairs"], "step": t["step"],
           "ratio_pairs_over_step": round(t["step_pairs"]["ms"] / t["step"]["ms"], 4),
           "kernels": {kname: count_kernels(fn) for kname, fn in arms.items()}}
    print(f"[bench_contrastive] step_pairs {t['step_pairs']['ms']} ms, step {t['step']['ms']} ms", file=sys.stderr)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--skip-step", action="store_true", help="the objective alone, without the cfg-2 training step")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_contrastive.py needs an MI355X"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "calls": args.calls,
           "objective": [bench_objective(R, N, d, args.calls, dev) for R, N, d in SHAPES]}
    if not args.skip_step:
        res["step"] = bench_step(max(args.calls // 2, 5), dev)
    text = json.dumps(res, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
