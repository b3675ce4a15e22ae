"""What gradient clipping and the EMA shadow cost: (a) the optimiser step alone, (b) the whole cfg-2 step.

    python scripts/bench_opt_step.py [--steps 10] [--warmup 3] [--rounds 3] [--iters 200] [--skip-step | --skip-alone]

(a) The launches of one optimiser step on flat buffers of n = 370 688 floats (bench.py's cfg-2: rank-4 q/k/v adapters of
12 + 12 blocks and the prompt ctx) and n = 3 934 208 (cfg-2 with ``q k v c_fc c_proj`` at r = 16), random contents, no
model: plain AdamW (1 launch), clip (3), EMA (1), clip + EMA (3), and the same four behind dynamic loss scaling (3, 5,
3, 5 launches).  The last launch of every arm is the one AdamW kernel through ``ops.adamw_ext``, with the records that are
off passed as None.  Per arm --iters back-to-back steps between two HIP events, --rounds times, the arms alternating;
microseconds per step: median, minimum and maximum over the rounds.  Back-to-back steps never wait for the host, as
inside a training step; what comes out is the larger of the device time and the time to issue the launches, so at the
small size (1.5 MB per buffer) expect a multiple of the per-launch issue time rather than a bandwidth figure.

(b) The cfg-2 step (ViT-B/32 fp32, 256 images + 403 captions, LoRA dropout 0.25: ``python bench.py``'s trainer) with the
options off, ``max_grad_norm=1.0`` only, ``ema_decay=0.999`` only and both, each arm on its own model, alternating in
one process (--rounds rounds of --steps steps after --warmup warm-ups, per-step HIP-event times): median, minimum and
maximum per arm.  The arm with the options off is the step ``python bench.py`` times; run that of the parent commit
and of this one alternately beside this script to place it inside the spread of the parent's runs.

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

LR, BETAS, EPS, WD = 2e-4, (0.9, 0.999), 1e-8, 1e-2
ARMS = {"none": {}, "clip": {"max_grad_norm": 1.0}, "ema": {"ema_decay": 0.999},
        "clip_ema": {"max_grad_norm": 1.0, "ema_decay": 0.999}}


def stats(xs, digits=3):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits), "max": round(max(xs), digits)}


class FlatStep:
    """The launch sequence of ``FlatStepTrainer._apply_update`` on bare buffers."""

    def __init__(self, dev, n, clip, ema, scaled):
        from clipfs import ops
        g = torch.Generator().manual_seed(n)
        self.p = (torch.randn(n, generator=g) * 0.05).to(dev)
        self.g = (torch.randn(n, generator=g) * 1e-2).to(dev)
        self.m, self.v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        self.scale = ops.new_scaler_state(65536.0, dev) if scaled else None
        if scaled:
            self.g.mul_(65536.0)
        self.clip = ops.new_clip_state(dev) if clip else None
        self.work = ops.grad_sumsq_work(n, dev) if clip else None
        self.shadow = self.p.clone() if ema else None
        self.t = 0
        self.launches = (2 if scaled else 0) + (2 if clip else 0) + 1

    def step(self):
        from clipfs import ops
        self.t += 1
        if self.scale is not None:
            ops.grads_nonfinite(self.g, self.scale)
            ops.scaler_decide(self.scale, LR, BETAS, 2.0, 0.5, 0)  # interval 0: the scale (and the buffer's meaning) stays
        if self.clip is not None:
            ops.grad_sumsq(self.g, self.work)
            ops.clip_decide(self.work, self.g.numel(), 1.0, self.clip, self.scale)
        ops.adamw_ext(self.p, self.g, self.m, self.v, self.t, LR, BETAS, EPS, WD, 1.0, self.scale, self.clip, self.shadow,
                      0.999 if self.shadow is not None else 0.0)


def alone(dev, n, args):
    arms = {}
    for scaled in (False, True):
        for name, kw in ARMS.items():
            arms[("scaled_" if scaled else "") + name] = FlatStep(dev, n, "max_grad_norm" in kw, "ema_decay" in kw, scaled)
    for a in arms.values():
        for _ in range(10):
            a.step()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, a in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                a.step()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(1e3 * e0.elapsed_time(e1) / args.iters)
    out = {k: dict(stats(t, 2), launches=arms[k].launches) for k, t in times.items()}
    out["unit"] = "microseconds per optimiser step"
    out["sample"] = f"{args.rounds} alternating rounds x {args.iters} back-to-back steps per arm"
    return out


def build(dev, **kw):
    """bench.py's cfg-2 trainer, rebuilt with the options (their buffers are made at construction)."""
    import bench
    import lora_train_vlp as L
    a = types.SimpleNamespace(model="b32", dropout=0.25, no_shard_text=True, serial_towers=False, trim_text=False,
                              precision="fp32")
    model, tr, cfg = bench.build_trainer(dev, a)
    tr = L.LoRATrainer(model, prompt_ctx=tr.prompt_ctx, shard_text=False, **kw)
    return model, tr, cfg


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


def whole_step(dev, args, batch=256, classes=403):
    from clipfs import synth
    runs = {k: build(dev, **kw) for k, kw in ARMS.items()}
    cfg = runs["none"][2]
    data = (synth.synth_images(batch, 224, seed=0).to(dev), synth.synth_captions(classes, 77, cfg.vocab_size, seed=1).to(dev),
            synth.synth_labels(batch, 374, seed=2).to(dev))
    for k in ARMS:
        runs[k][0].train()
        time_steps(runs[k][1], data, batch, args.warmup)
    times = {k: [] for k in ARMS}
    for _ in range(args.rounds):
        for k in ARMS:
            times[k] += time_steps(runs[k][1], data, batch, args.steps)
    out = {k: {f"{s}_ms": v for s, v in stats(t).items()} for k, t in times.items()}
    for k in ("clip", "ema", "clip_ema"):
        out[k]["over_none_median"] = round(out[k]["median_ms"] / out["none"]["median_ms"], 4)
    tr = runs["clip_ema"][1]
    out["clip_ema"]["last_grad_norm"], out["clip_ema"]["last_clip_coef"] = tr.last_grad_norm, tr.last_clip_coef
    out["flat_floats"] = tr.flat.numel
    out["sample"] = f"{args.rounds} alternating rounds x {args.steps} steps per arm after {args.warmup} warm-ups"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200, help="back-to-back optimiser steps per timing of part (a)")
    ap.add_argument("--skip-step", action="store_true", help="part (a) only")
    ap.add_argument("--skip-alone", action="store_true", help="part (b) only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_opt_step.py needs an MI355X")
    dev = torch.device("cuda:0")
    out = {}
    if not args.skip_alone:
        out["optimiser_step_alone"] = {str(n): alone(dev, n, args) for n in (370688, 3934208)}
    if not args.skip_step:
        out["cfg2_step_b32_fp32_256x403"] = whole_step(dev, args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
