"""Step time of the cfg-2 step with shallow prompts vs deep prompts (IVLP vision_depth = language_depth = 9).

    python scripts/bench_deep_prompts.py [--steps 10] [--warmup 3] [--rounds 3] [--depth 9]

Step: ViT-B/32, 256 images + 403 captions, LoRA q/k/v r=4 with dropout 0.25 on every block, 4 prompt ctx tokens and
4 VPT tokens trained, class-sharded text off (one GPU), the bench.py trainer settings.  "shallow" is that step as it
is today; "deep" adds design_details {"deep_prompts": True, "vision_depth": depth, "language_depth": depth}, whose
blocks 1 ... depth-1 of both towers each train a [4, width] prompt (written into the block input in the forward, its
gradient harvested in the backward).  The two models are timed in interleaved rounds (median of per-step HIP-event
times).  Prints one JSON object."""
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


def build(dev, depth):
    import lora_train_vlp as L
    from clipfs import synth
    from jclip.model import build_model
    dd = {"vision_ctx": 4, "language_ctx": 4}
    if depth > 1:
        dd.update(deep_prompts=True, vision_depth=depth, language_depth=depth)
    model = build_model(synth.synth_state_dict(synth.VIT_B32, seed=1234), design_details=dd, device=dev)
    largs = types.SimpleNamespace(encoder="both", position="all", backbone="ViT-B/32", params=["q", "k", "v"], r=4,
                                  alpha=1, dropout_rate=0.25)
    L.apply_lora(largs, model)
    L.mark_only_lora_as_trainable(model)
    model.visual.VPT.requires_grad_(True)
    for n, p in model.named_parameters():
        if n.endswith(".VPT_shallow"):
            p.requires_grad_(True)
    ids = torch.tensor([320, 1125, 539, 320], device=dev)
    ctx = torch.nn.Parameter(model.token_embedding.weight.data[ids].clone())
    model.train()
    return model, L.LoRATrainer(model, prompt_ctx=ctx, shard_text=False)


def time_steps(tr, img, cap, tgt, n):
    out = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        tr.step(img, cap, tgt)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--depth", type=int, default=9)
    args = ap.parse_args()
    from clipfs import synth
    dev = torch.device("cuda:0")
    img = synth.synth_images(256, 224, seed=0).to(dev)
    cap = synth.synth_captions(403, 77, synth.VIT_B32.vocab_size, seed=1).to(dev)
    tgt = synth.synth_labels(256, 403, seed=2).to(dev)
    runs = {"shallow": build(dev, 1), "deep": build(dev, args.depth)}
    times = {k: [] for k in runs}
    for _, tr in runs.values():
        time_steps(tr, img, cap, tgt, args.warmup)
    for _ in range(args.rounds):
        for k, (_, tr) in runs.items():
            times[k] += time_steps(tr, img, cap, tgt, args.steps)
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {k: {"median_ms": round(med[k], 3), "min_ms": round(min(times[k]), 3), "plan": runs[k][1].last_plan,
               "trained_floats": runs[k][1].flat.numel} for k in runs}
    print(json.dumps({"depth": args.depth, "runs": out, "deep_overhead": round(med["deep"] / med["shallow"] - 1, 4),
                      "sample": f"{args.rounds} interleaved rounds x {args.steps} steps per model after {args.warmup} "
                                f"warm-ups"}))


if __name__ == "__main__":
    main()
