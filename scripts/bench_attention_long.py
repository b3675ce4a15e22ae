"""Measurements at ViT-L/14@336's sequence length (577 tokens, 16 heads) for the fp16 storage mode.

    python scripts/bench_attention_long.py --kernels [--batch 64] [--rounds 7] [--json OUT]
        attention forward and backward: the long-sequence f16 MFMA kernels (ops.attention_f16_fwd / _bwd) against the
        streaming fp32 kernels (ops.attention_fwd / _bwd, what an fp16-mode tower ran past 288 tokens before), interleaved
        round by round in ONE process; median and minimum per direction.
    python scripts/bench_attention_long.py --step [--batch 64] [--steps 5] [--warmup 3] [--json OUT]
        one ViT-L/14@336 train step in fp16 mode (full depth 24 + 12, rank-16 LoRA on q, k, v, synthetic weights, 403
        captions): uses the engine's public API only, so the same file times any checkout of the project -- run it from
        two checkouts alternately on one card to compare them.
Each mode prints one JSON line (and writes it to --json)."""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jittor-clip-fewshot_amd"))
sys.path.insert(0, ROOT)

SEQ, HEADS = 577, 16


def _timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us


def kernels(args):
    from clipfs import ops
    dev = torch.device("cuda:0")
    B, H, L = args.batch, HEADS, SEQ
    g = torch.Generator().manual_seed(1)
    qkv = torch.randn(B * L, 3 * H * 64, generator=g).to(dev)  # random data: zeros would flatter the softmax
    dout = torch.randn(B * L, H * 64, generator=g).to(dev)
    out32, lse32 = ops.attention_fwd(qkv, B, L, H, False, want_lse=True)
    out16, lse16 = ops.attention_f16_fwd(qkv, B, L, H)
    arms = {
        "fwd_fp32_streaming": lambda: ops.attention_fwd(qkv, B, L, H, False, want_lse=True),
        "fwd_f16_long": lambda: ops.attention_f16_fwd(qkv, B, L, H),
        "bwd_fp32_streaming": lambda: ops.attention_bwd(qkv, dout, B, L, H, False, out=out32, lse=lse32),
        "bwd_f16_long": lambda: ops.attention_f16_bwd(qkv, dout, out16, lse16, B, L, H),
    }
    for fn in arms.values():  # warm-up: first-launch costs and clocks
        fn()
        fn()
    torch.cuda.synchronize()
    us = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, fn in arms.items():
            us[k].append(_timed(fn, 3))
    fl = 4 * L * L * 64 * B * H  # forward; the backward is priced at 2.5 x
    res = {"mode": "kernels", "batch": B, "heads": H, "seq": L, "rounds": args.rounds, "iters_per_round": 3, "unit": "us",
           "device": torch.cuda.get_device_name(0)}
    for k, v in us.items():
        f = fl * (2.5 if k.startswith("bwd") else 1.0)
        res[k] = {"median": round(statistics.median(v), 1), "min": round(min(v), 1),
                  "tflops_at_median": round(f / statistics.median(v) / 1e6, 1)}
    res["fwd_speedup_median"] = round(res["fwd_fp32_streaming"]["median"] / res["fwd_f16_long"]["median"], 2)
    res["bwd_speedup_median"] = round(res["bwd_fp32_streaming"]["median"] / res["bwd_f16_long"]["median"], 2)
    return res


def step(args):
    import lora_train_vlp as L
    from clipfs import synth
    from jclip.model import build_model
    dev = torch.device("cuda:0")
    cfg = dataclasses.replace(synth.VIT_L14, image_resolution=336)
    assert cfg.vision_tokens == SEQ
    sd = synth.synth_state_dict(cfg, seed=1234)
    model = build_model(sd, device=dev)
    del sd
    largs = types.SimpleNamespace(encoder="both", position="all", backbone="ViT-L/14", params=["q", "k", "v"], r=16, alpha=1,
                                  dropout_rate=0.25)
    layers = L.apply_lora(largs, model)
    lw = synth.synth_lora(cfg, 16, seed=5, vision_blocks=range(21))
    names = {"q": "q_proj", "k": "k_proj", "v": "v_proj"}
    with torch.no_grad():
        for i, layer in enumerate(layers):
            for p in "qkv":
                m = getattr(layer, names[p])
                m.w_lora_A.copy_(torch.from_numpy(lw[f"layer_{i}"][names[p]]["w_lora_A"]))
                m.w_lora_B.copy_(torch.from_numpy(lw[f"layer_{i}"][names[p]]["w_lora_B"]))
    L.mark_only_lora_as_trainable(model)
    model.train()
    tr = L.LoRATrainer(model)
    model.engine.precision = "fp16"
    B, Cn = args.batch, 403
    images = synth.synth_images(B, 336, seed=0).to(dev)
    labels = synth.synth_labels(B, 374, seed=2).to(dev)
    captions = synth.synth_captions(Cn, 77, cfg.vocab_size, seed=1).to(dev)

    def one():
        tr.flat.zero_grad()
        tr.forward_backward(images, captions, labels, 1, B)
        tr.optimizer_step()

    for _ in range(args.warmup):
        one()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        one()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"mode": "step", "model": "ViT-L/14@336 (577 vision tokens), 24 + 12 blocks, LoRA r=16 on q,k,v, fp16 storage mode",
            "images": B, "captions": Cn, "steps": args.steps, "warmup": args.warmup, "unit": "ms",
            "ms_per_step_median": round(statistics.median(ms), 2), "ms_per_step_min": round(min(ms), 2),
            "images_per_s_at_median": round(B / statistics.median(ms) * 1e3, 1), "tree": args.label or ROOT,
            "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--label", default="", help="name of the checkout being timed (recorded in the JSON line)")
    ap.add_argument("--json", metavar="OUT")
    args = ap.parse_args()
    if args.kernels == args.step:
        ap.error("give exactly one of --kernels / --step")
    res = kernels(args) if args.kernels else step(args)
    line = json.dumps(res)
    print(line, flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
