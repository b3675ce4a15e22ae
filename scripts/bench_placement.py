"""Step time of the cfg-2 step per adapter layout, with the gradient floor (Engine.prune_backward) on and off.

    python scripts/bench_placement.py [--steps 10] [--warmup 3] [--rounds 3] [--ctx]

Step: ViT-B/32, 256 images + 403 captions, LoRA q/k/v r=4 with dropout 0.25, class-sharded text off (one GPU), the
bench.py trainer settings; layouts encoder in {both, text, vision} x position in {all, up, bottom}.  Without --ctx no
prompt tokens train (with them the text tower's input needs a gradient and its floor is always 0).  Each layout is one
model; prune_backward on / off are timed in interleaved rounds on it (median of per-step HIP-event times), then the
model is freed.  Prints one JSON object."""
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


def build(dev, encoder, position, with_ctx):
    import lora_train_vlp as L
    from clipfs import synth
    from jclip.model import build_model
    model = build_model(synth.synth_state_dict(synth.VIT_B32, seed=1234), device=dev)
    largs = types.SimpleNamespace(encoder=encoder, position=position, backbone="ViT-B/32", params=["q", "k", "v"], r=4,
                                  alpha=1, dropout_rate=0.25)
    L.apply_lora(largs, model)
    L.mark_only_lora_as_trainable(model)
    ctx = None
    if with_ctx:
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
    ap.add_argument("--ctx", action="store_true", help="train 4 prompt ctx tokens as well (cfg-2 of bench.py)")
    args = ap.parse_args()
    from clipfs import synth
    dev = torch.device("cuda:0")
    img = synth.synth_images(256, 224, seed=0).to(dev)
    cap = synth.synth_captions(403, 77, synth.VIT_B32.vocab_size, seed=1).to(dev)
    tgt = synth.synth_labels(256, 403, seed=2).to(dev)
    res = {}
    for encoder in ("both", "text", "vision"):
        for position in ("all", "up", "bottom"):
            model, tr = build(dev, encoder, position, args.ctx)
            times = {True: [], False: []}
            for prune in (True, False):
                model.engine.prune_backward = prune
                time_steps(tr, img, cap, tgt, args.warmup)
            for _ in range(args.rounds):
                for prune in (True, False):
                    model.engine.prune_backward = prune
                    times[prune] += time_steps(tr, img, cap, tgt, args.steps)
            model.engine.prune_backward = True
            tr.step(img, cap, tgt)
            med = {k: statistics.median(v) for k, v in times.items()}
            res[f"{encoder}/{position}"] = {"plan": tr.last_plan, "pruned_ms": round(med[True], 3),
                                            "full_ms": round(med[False], 3),
                                            "pruned_min_ms": round(min(times[True]), 3),
                                            "full_min_ms": round(min(times[False]), 3)}
            del model, tr
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
    base = res["both/all"]["pruned_ms"]
    for v in res.values():
        v["vs_both_all"] = round(v["pruned_ms"] / base, 4)
        v["saved_fraction"] = round(1 - v["pruned_ms"] / v["full_ms"], 4)
    print(json.dumps({"ctx": args.ctx, "layouts": res,
                      "sample": f"{args.rounds} interleaved rounds x {args.steps} steps per setting after "
                                f"{args.warmup} warm-ups"}))


if __name__ == "__main__":
    main()
