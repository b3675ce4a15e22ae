"""Cost of LoRA on the MLP linears: the cfg-2 step with params q k v against q k v c_fc c_proj, and the rectangular adapter
products alone at the towers' shapes.

    python scripts/bench_mlp_lora.py [--ranks 4 16] [--steps 10] [--warmup 3] [--rounds 3] [--reps 20] [--no-step]

Step: ViT-B/32, 256 images + 403 captions, adapters of rank r on every block with dropout 0.25 (A ~ U(+-1/sqrt(in)),
B ~ N(0, 0.02^2)), 4 prompt ctx tokens, class-sharded text off (one GPU), otherwise the bench.py trainer settings.  The
four variants (two parameter sets x the ranks) are timed in interleaved rounds (median of per-step HIP-event times);
``step_ratio`` is the MLP variant over the q/k/v-only step at the same rank.

Products: clipfs_lora_down and clipfs_lora_bwd_xact on 12 800 rows x 768 <-> 3072 (the image tower) and 31 031 rows x
512 <-> 2048 (the text tower's dense rows), p 0.25: the c_fc adapter (in d, out 4d, reads h2) and the c_proj adapter (in 4d,
out d, reads the pre-activation with QuickGELU on load; its in-place gelu' pass over [rows, 4d] is timed beside it).  Each is
timed alone (median over --reps HIP-event timed calls) against the HBM floor of the bytes it must move.  Prints one JSON
object."""
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

HBM_BYTES_S = 8.0e12  # MI355X HBM3E peak
PARAM_SETS = {"qkv": ["q", "k", "v"], "qkv+mlp": ["q", "k", "v", "c_fc", "c_proj"]}


def build(dev, r, params):
    import lora_train_vlp as L
    from clipfs import synth
    from jclip.model import build_model
    cfg = synth.VIT_B32
    model = build_model(synth.synth_state_dict(cfg, seed=1234), device=dev)
    largs = types.SimpleNamespace(encoder="both", position="all", backbone="ViT-B/32", params=list(params), r=r, alpha=1,
                                  dropout_rate=0.25)
    layers = L.apply_lora(largs, model)
    g = torch.Generator().manual_seed(5)
    names = {"q": "q_proj", "k": "k_proj", "v": "v_proj"}
    with torch.no_grad():
        for layer in layers:
            for tok in params:
                m = getattr(layer, names.get(tok, tok))
                m.w_lora_B.copy_(torch.randn(m.w_lora_B.shape, generator=g) * 0.02)
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


def products(dev, rows, d, r, reps):
    """the products of the two MLP adapters of one block at ``rows`` x (d <-> 4d)"""
    from clipfs import _lib, ops
    p, seed, f = 0.25, 0x5EED, 4
    g = torch.Generator(device=dev).manual_seed(r)
    res = {}
    for name, fin, fout, x_act in (("c_fc", d, 4 * d, False), ("c_proj", 4 * d, d, True)):
        x = torch.randn(rows, fin, device=dev, generator=g)
        A = torch.randn(r, fin, device=dev, generator=g) * fin ** -0.5
        B = torch.randn(fout, r, device=dev, generator=g) * 0.02
        dy = torch.randn(rows, fout, device=dev, generator=g)
        dA, dB, dx = torch.zeros_like(A), torch.zeros_like(B), torch.zeros_like(x)
        t = ops.lora_down(x, A, r, 1, p=p, seed=seed)
        down_ms = time_call(lambda: ops.lora_down(x, A, r, 1, p=p, seed=seed), reps)
        bwd_ms = time_call(lambda: ops.lora_bwd_rect(dy, x, t, A, B, dA, dB, dx=dx, scale=0.5, p=p, seed=seed, x_act=x_act), reps)
        work = _lib.load().clipfs_lora_bwd_work_floats2(rows, fin, fout, r, 1)
        # bytes each must move: down reads x and writes t; the backward reads dy twice (dt, dB), x once (dA), t and dt, reads
        # and writes dx, and writes + reads the slice partials (counted from the work bound)
        down_bytes = f * rows * fin + f * rows * r
        bwd_bytes = 2 * f * rows * fout + f * rows * fin + 3 * f * rows * r + 2 * f * rows * fin + 2 * f * work
        res[name] = {}
        for k, ms, nbytes in (("down", down_ms, down_bytes), ("bwd", bwd_ms, bwd_bytes)):
            res[name][k] = {"ms": round(ms, 4), "GB_s": round(nbytes / (ms * 1e-3) / 1e9, 1),
                            "hbm_floor_ms": round(nbytes / HBM_BYTES_S * 1e3, 4)}
        res[name]["work_MB"] = round(4 * work / 2 ** 20, 1)
        if x_act:
            gelu_ms = time_call(lambda: ops.gelu_bwd_inplace(dx, x), reps)
            res["gelu_bwd"] = {"ms": round(gelu_ms, 4), "hbm_floor_ms": round(3 * f * rows * fin / HBM_BYTES_S * 1e3, 4)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-step", action="store_true", help="time the adapter products only")
    args = ap.parse_args()
    from clipfs import synth
    dev = torch.device("cuda:0")
    out = {"ranks": args.ranks}
    out["products"] = {r: {f"{rows}x{d}<->{4 * d}": products(dev, rows, d, r, args.reps)
                           for rows, d in ((12800, 768), (31031, 512))} for r in args.ranks}
    if not args.no_step:
        img = synth.synth_images(256, 224, seed=0).to(dev)
        cap = synth.synth_captions(403, 77, synth.VIT_B32.vocab_size, seed=1).to(dev)
        tgt = synth.synth_labels(256, 403, seed=2).to(dev)
        runs = {(name, r): build(dev, r, params) for r in args.ranks for name, params in PARAM_SETS.items()}
        times = {k: [] for k in runs}
        for _, tr in runs.values():
            time_steps(tr, img, cap, tgt, args.warmup)
        for _ in range(args.rounds):
            for k, (_, tr) in runs.items():
                times[k] += time_steps(tr, img, cap, tgt, args.steps)
        med = {k: statistics.median(v) for k, v in times.items()}
        out["step"] = {f"{name} r={r}": {"median_ms": round(med[(name, r)], 3), "min_ms": round(min(times[(name, r)]), 3),
                                         "trained_floats": runs[(name, r)][1].flat.numel} for name, r in runs}
        out["step_ratio"] = {f"r={r}": round(med[("qkv+mlp", r)] / med[("qkv", r)], 4) for r in args.ranks}
        out["sample"] = f"{args.rounds} interleaved rounds x {args.steps} steps per variant after {args.warmup} warm-ups"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
