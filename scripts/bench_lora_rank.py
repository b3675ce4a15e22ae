"""Cost of the LoRA rank: the cfg-2 step at r = 4, 16, 32, 64 and the adapter products alone at the towers' shapes.

    python scripts/bench_lora_rank.py [--ranks 4 16 32 64] [--steps 10] [--warmup 3] [--rounds 3] [--reps 20]

Step: ViT-B/32, 256 images + 403 captions, LoRA q/k/v r on every block with dropout 0.25 (A ~ U(+-1/sqrt(in)),
B ~ N(0, 0.02^2), seed 5), 4 prompt ctx tokens, class-sharded text off (one GPU), otherwise the bench.py trainer
settings.  The ranks are timed in interleaved rounds (median of per-step HIP-event times).

Products: clipfs_lora_down (with keep bits) and the three-launch backward (clipfs_lora_bwd reading them) on
12 800 x 768 (the image tower's rows) and 31 031 x 512 (the text tower's dense rows), nseg 3, p 0.25.  Each is timed
alone (median over --reps HIP-event timed calls) and reported against two floors: the bytes it must move at the HBM
peak, and its FLOPs at the fp32-MFMA peak.  Prints one JSON object."""
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

HBM_BYTES_S = 8.0e12          # MI355X HBM3E peak
FP32_MFMA_FLOP_S = 157.3e12   # MI355X dense fp32 matrix peak


def build(dev, r):
    import lora_train_vlp as L
    from clipfs import synth
    from jclip.model import build_model
    cfg = synth.VIT_B32
    model = build_model(synth.synth_state_dict(cfg, seed=1234), device=dev)
    largs = types.SimpleNamespace(encoder="both", position="all", backbone="ViT-B/32", params=["q", "k", "v"], r=r,
                                  alpha=1, dropout_rate=0.25)
    layers = L.apply_lora(largs, model)
    lw = synth.synth_lora(cfg, r, seed=5)
    names = {"q": "q_proj", "k": "k_proj", "v": "v_proj"}
    with torch.no_grad():
        for i, layer in enumerate(layers):
            for pr in "qkv":
                m = getattr(layer, names[pr])
                m.w_lora_A.copy_(torch.from_numpy(lw[f"layer_{i}"][names[pr]]["w_lora_A"]))
                m.w_lora_B.copy_(torch.from_numpy(lw[f"layer_{i}"][names[pr]]["w_lora_B"]))
    L.mark_only_lora_as_trainable(model)
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


def time_call(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out)


def products(dev, rows, width, r, reps):
    """the adapter products of one q/k/v adapter (nseg 3, dropout with keep bits) at one shape"""
    from clipfs import ops
    nseg, p, seed = 3, 0.25, 0x5EED
    g = torch.Generator(device=dev).manual_seed(r)
    x = torch.randn(rows, width, device=dev, generator=g)
    A = torch.randn(nseg * r, width, device=dev, generator=g) * width ** -0.5
    B = torch.randn(nseg * width, r, device=dev, generator=g) * 0.02
    dy = torch.randn(rows, nseg * width, device=dev, generator=g)
    kb = ops.lora_keep_bits(rows, width, dev)
    dA, dB, dx = torch.zeros_like(A), torch.zeros_like(B), torch.zeros_like(x)
    t = ops.lora_down(x, A, r, nseg, p=p, seed=seed, keep_bits=kb)
    down_ms = time_call(lambda: ops.lora_down(x, A, r, nseg, p=p, seed=seed, keep_bits=kb), reps)
    bwd_ms = time_call(lambda: ops.lora_bwd(dy, x, t, A, B, dA, dB, dx=dx, scale=0.5, p=p, seed=seed, keep_bits=kb), reps)
    f, M, d, k = 4, rows, width, nseg * r
    # bytes each must move: down reads x and writes t + keep bits; the backward reads dy twice (dt, dB), x and the keep
    # bits once (dA), dt, reads and writes dx, and writes + reads the slice partials (counted from the work bound)
    from clipfs import _lib
    work = _lib.load().clipfs_lora_bwd_work_floats(rows, width, r, nseg)
    down_bytes = f * M * d + f * M * k + 2 * M * d // 4
    bwd_bytes = 2 * f * M * nseg * d + f * M * d + 2 * M * d // 4 + 2 * f * M * k + 2 * f * M * d + 2 * f * work
    down_flop = 2 * M * d * k
    bwd_flop = 4 * 2 * M * d * k  # dt, dB, dA, dx
    res = {}
    for name, ms, nbytes, flop in (("down", down_ms, down_bytes, down_flop), ("bwd", bwd_ms, bwd_bytes, bwd_flop)):
        s = ms * 1e-3
        res[name] = {"ms": round(ms, 4), "GB_s": round(nbytes / s / 1e9, 1), "TFLOP_s": round(flop / s / 1e12, 2),
                     "hbm_floor_ms": round(nbytes / HBM_BYTES_S * 1e3, 4),
                     "mfma_floor_ms": round(flop / FP32_MFMA_FLOP_S * 1e3, 4)}
    res["work_MB"] = round(4 * work / 2 ** 20, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", type=int, nargs="+", default=[4, 16, 32, 64])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-step", action="store_true", help="time the adapter products only")
    args = ap.parse_args()
    from clipfs import synth
    dev = torch.device("cuda:0")
    out = {"ranks": args.ranks}
    prod = {}
    for r in args.ranks:
        prod[r] = {f"{rows}x{width}": products(dev, rows, width, r, args.reps) for rows, width in ((12800, 768), (31031, 512))}
    out["products"] = prod
    if not args.no_step:
        img = synth.synth_images(256, 224, seed=0).to(dev)
        cap = synth.synth_captions(403, 77, synth.VIT_B32.vocab_size, seed=1).to(dev)
        tgt = synth.synth_labels(256, 403, seed=2).to(dev)
        runs = {r: build(dev, r) for r in args.ranks}
        times = {r: [] for r in runs}
        for _, tr in runs.values():
            time_steps(tr, img, cap, tgt, args.warmup)
        for _ in range(args.rounds):
            for r, (_, tr) in runs.items():
                times[r] += time_steps(tr, img, cap, tgt, args.steps)
        med = {r: statistics.median(v) for r, v in times.items()}
        out["step"] = {r: {"median_ms": round(med[r], 3), "min_ms": round(min(times[r]), 3),
                           "trained_floats": runs[r][1].flat.numel} for r in runs}
        if 16 in med:
            out["step_ratio_vs_r16"] = {r: round(med[r] / med[16], 4) for r in med}
        out["sample"] = f"{args.rounds} interleaved rounds x {args.steps} steps per rank after {args.warmup} warm-ups"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
