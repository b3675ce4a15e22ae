"""Loss scaling in the fp16 storage mode: (a) how much of the gradient f16 loses without it, (b) what it costs per step.

    python scripts/bench_loss_scale.py [--steps 10] [--warmup 3] [--rounds 3] [--skip-cost | --skip-underflow]

(a) ViT-L/14, rank-16 q/k/v adapters (bench.py's cfg-5 model) at full depth (24 + 12 blocks; 12 + 12, then 6 + 6 if
that runs out of memory: the output says which), 128 images + 403 captions, no dropout
(eval mode), prompt ctx: ONE forward_backward on identical inputs per arm -- precision "fp32" (the yardstick), "fp16"
unscaled, "fp16" with loss_scale="dynamic" once the scale has settled (steps at lr = 0 and weight decay 0, which leave
the parameters bitwise alone, until one is not skipped).  For each fp16 arm against the fp32 gradient: maximum and RMS
error relative to the largest fp32 entry, and the share of entries that are exactly zero where fp32's is not, over the
whole flat buffer and per tower.  Then the same with global_batch = 1024 (one rank's share of the reference's batch).

(b) step time with loss_scale="dynamic" against None, each arm on its own model, alternating in one process (--rounds
rounds of --steps steps after --warmup warm-ups, per-step HIP-event times): the cfg-5 step (ViT-L/14 fp16, 128 + 403)
and the cfg-2 step (ViT-B/32 fp32, 256 + 403), LoRA dropout 0.25 as in bench.py.  Median, minimum and maximum per arm.

Prints one JSON object."""
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


def build(dev, model_name, precision, loss_scale, lr=2e-4, wd=1e-2, depth=None):
    """bench.py's trainer for the model, rebuilt with the scaler settings (the record is made at construction).
    ``depth`` = (vision, text) layers builds a shallower ViT-L/14 (part (a) when the full depth does not fit)."""
    import dataclasses
    import bench
    import lora_train_vlp as L
    from clipfs import synth
    a = types.SimpleNamespace(model=model_name, dropout=0.25, no_shard_text=True, serial_towers=False, trim_text=False,
                              precision=precision)
    full = synth.VIT_L14
    if depth is not None:
        synth.VIT_L14 = dataclasses.replace(full, vision_layers=depth[0], transformer_layers=depth[1])
    try:
        model, tr, cfg = bench.build_trainer(dev, a)
    finally:
        synth.VIT_L14 = full
    tr = L.LoRATrainer(model, lr=lr, weight_decay=wd, prompt_ctx=tr.prompt_ctx, shard_text=False, loss_scale=loss_scale)
    return model, tr, cfg


def inputs(dev, cfg, batch, classes=403, label_classes=374):
    from clipfs import synth
    return (synth.synth_images(batch, 224, seed=0).to(dev),
            synth.synth_captions(classes, 77, cfg.vocab_size, seed=1).to(dev),
            synth.synth_labels(batch, label_classes, seed=2).to(dev))


def text_floats(model):
    """Number of leading floats of the flat buffer that belong to the text tower's adapters."""
    return sum(p.numel() for blk in model.transformer.resblocks if getattr(blk.attn, "is_lora_mha", False)
               for _, p, _ in blk.attn.stacked())


def compare(g16, g32, n_text, n_lora):
    peak = g32.abs().max().item()
    out = {}
    for name, sl in (("all", slice(None)), ("text_adapters", slice(0, n_text)), ("vision_adapters", slice(n_text, n_lora))):
        a, b = g16[sl].double(), g32[sl].double()
        d = (a - b).abs()
        nz = b != 0
        out[name] = {"max_err_rel_peak": d.max().item() / peak, "rms_err_rel_peak": d.pow(2).mean().sqrt().item() / peak,
                     "zero_where_fp32_is_not": ((a == 0) & nz).sum().item() / max(1, nz.sum().item()),
                     "fp32_rms_rel_peak": b.pow(2).mean().sqrt().item() / peak}
    out["fp32_peak"] = peak
    return out


def settle(tr, data, gb, limit=24):
    """Run lr = 0 steps until one is applied: the scale the dynamic scaler settles at for these inputs."""
    for _ in range(limit):
        before = tr.skipped_steps
        tr.step(*data, 1, gb)
        if tr.skipped_steps == before:
            return tr.loss_scale_value
    raise RuntimeError("the dynamic scale did not settle")


def underflow(dev):
    full = (24, 12)
    for depth in (full, (12, 12), (6, 6)):
        try:
            return underflow_at(dev, None if depth == full else depth)
        except torch.OutOfMemoryError:
            print(f"[bench_loss_scale] depth {depth} does not fit in memory, trying a shallower model", file=sys.stderr)
            torch.cuda.empty_cache()
    raise SystemExit("part (a) does not fit at any of the depths tried")


def underflow_at(dev, depth):
    import lora_train_vlp as L
    model, tr0, cfg = build(dev, "l14", "fp32", None, depth=depth)
    model.eval()  # no LoRA dropout: the three arms see the same function
    data = inputs(dev, cfg, 128)
    ctx = tr0.prompt_ctx
    n_text = text_floats(model)
    res = {"depth": {"vision": cfg.vision_layers, "text": cfg.transformer_layers, "full": depth is None},
           "shapes": "ViT-L/14, 128 images + 403 captions, q/k/v adapters r = 16, prompt ctx, dropout 0"}
    for gb in (128, 1024):
        grads = {}
        for arm, prec, ls in (("fp32", "fp32", None), ("fp16", "fp16", None), ("fp16_dynamic", "fp16", "dynamic")):
            model.engine.precision = prec
            tr = L.LoRATrainer(model, lr=0.0, weight_decay=0.0, prompt_ctx=ctx, shard_text=False, loss_scale=ls)
            n_lora = tr.flat.numel - ctx.numel()
            scale = 1.0
            if ls is not None:
                scale = settle(tr, data, gb)
                res.setdefault("settled_scale", {})[str(gb)] = scale
                res.setdefault("skipped_while_settling", {})[str(gb)] = tr.skipped_steps
            tr.flat.zero_grad()
            tr.forward_backward(*data, 1, gb)
            torch.cuda.synchronize()
            grads[arm] = tr.flat.grads / scale
            del tr
        res[f"global_batch_{gb}"] = {arm: compare(grads[arm], grads["fp32"], n_text, n_lora)
                                     for arm in ("fp16", "fp16_dynamic")}
    return res


def time_steps(tr, data, gb, n):
    out = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        tr.step(*data, 1, gb)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def cost(dev, model_name, precision, batch, args):
    arms = {"none": None, "dynamic": "dynamic"}
    runs = {k: build(dev, model_name, precision, v) for k, v in arms.items()}
    data = inputs(dev, runs["none"][2], batch)
    for k in arms:
        runs[k][0].train()
        time_steps(runs[k][1], data, batch, args.warmup)
    skipped0 = runs["dynamic"][1].skipped_steps
    times = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k in arms:
            times[k] += time_steps(runs[k][1], data, batch, args.steps)
    tr = runs["dynamic"][1]
    out = {k: {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}
           for k, t in times.items()}
    out["dynamic_over_none_median"] = round(out["dynamic"]["median_ms"] / out["none"]["median_ms"], 4)
    out["dynamic_arm"] = {"scale_at_end": tr.loss_scale_value, "skipped_in_warmup": skipped0,
                          "skipped_in_timed_steps": tr.skipped_steps - skipped0, "optimizer_steps": tr.optimizer_steps}
    out["sample"] = f"{args.rounds} alternating rounds x {args.steps} steps per arm after {args.warmup} warm-ups"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-cost", action="store_true", help="part (a) only")
    ap.add_argument("--skip-underflow", action="store_true", help="part (b) only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_loss_scale.py needs an MI355X")
    dev = torch.device("cuda:0")
    out = {}
    if not args.skip_underflow:
        out["underflow"] = underflow(dev)
        torch.cuda.empty_cache()
    if not args.skip_cost:
        out["cost_cfg5_l14_fp16_128x403"] = cost(dev, "l14", "fp16", 128, args)
        torch.cuda.empty_cache()
        out["cost_cfg2_b32_fp32_256x403"] = cost(dev, "b32", "fp32", 256, args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
