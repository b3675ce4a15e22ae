"""Cost of bias training (mark_only_lora_as_trainable(model, bias)) in the cfg-2 step, and the column-sum kernel's
effective bandwidth.

    python scripts/bench_bias.py [--steps 10] [--warmup 3] [--rounds 3]

Step: ViT-B/32, 256 images + 403 captions, LoRA q/k/v r=4 with dropout 0.25, prompt ctx, class-sharded text off (one
GPU), the bench.py trainer; bias='none' | 'lora_only' | 'all' each on its own model, timed in interleaved rounds
(median of per-step HIP-event times).  Kernel: clipfs_bias_grad (both passes) on the tower shapes of DESIGN.md
section 9, bytes = rows * cols * 4 read once.  Prints one JSON object."""
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


def build(dev, bias):
    import bench
    import lora_train_vlp as L
    a = types.SimpleNamespace(model="b32", dropout=0.25, no_shard_text=True, serial_towers=False, trim_text=False,
                              precision="fp32")
    model, tr, cfg = bench.build_trainer(dev, a)
    # rebuild the trainer with the bias flags set (the flat buffer is assembled at construction)
    L.mark_only_lora_as_trainable(model, bias)
    tr = L.LoRATrainer(model, prompt_ctx=tr.prompt_ctx, shard_text=False)
    return model, tr, cfg


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


def kernel_bw(dev, shapes, iters=50):
    from clipfs import ops
    res = {}
    for rows, cols in shapes:
        x = torch.randn(rows, cols, device=dev)
        out = torch.zeros(cols, device=dev)
        work = torch.empty(max(1, ops._lib.load().clipfs_bias_grad_work_floats(rows, cols)), device=dev)
        for _ in range(5):
            ops.bias_grad(x, out, work=work)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            ops.bias_grad(x, out, work=work)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / iters
        res[f"{rows}x{cols}"] = {"us": round(us, 2), "TB/s": round(rows * cols * 4 / us / 1e6, 2)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    from clipfs import synth
    dev = torch.device("cuda:0")
    out = {"kernel": kernel_bw(dev, [(12800, 768), (12800, 2304), (12800, 3072), (31031, 512), (31031, 1536),
                                     (31031, 2048), (256, 3072), (403, 2048)])}
    modes = ("none", "lora_only", "all")
    runs = {m: build(dev, m) for m in modes}
    img = synth.synth_images(256, 224, seed=0).to(dev)
    cap = synth.synth_captions(403, 77, synth.VIT_B32.vocab_size, seed=1).to(dev)
    tgt = synth.synth_labels(256, 403, seed=2).to(dev)
    for m in modes:
        time_steps(runs[m][1], img, cap, tgt, args.warmup)
    times = {m: [] for m in modes}
    for _ in range(args.rounds):
        for m in modes:
            times[m] += time_steps(runs[m][1], img, cap, tgt, args.steps)
    med = {m: statistics.median(t) for m, t in times.items()}
    out["step_ms_median"] = {m: round(v, 3) for m, v in med.items()}
    out["step_ms_min"] = {m: round(min(t), 3) for m, t in times.items()}
    out["ratio_vs_none"] = {m: round(med[m] / med["none"], 4) for m in modes}
    out["trained_bias_floats"] = {m: runs[m][1].flat.numel - runs[m][1].flat.bias_offset for m in modes}
    out["sample"] = f"{args.rounds} interleaved rounds x {args.steps} steps per mode after {args.warmup} warm-ups"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
