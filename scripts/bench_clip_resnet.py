"""CLIP ModifiedResNet (RN50) image tower on the HIP engine: forward rate, where the time goes, and one training step.

    python scripts/bench_clip_resnet.py [--batch 256] [--forwards 24] [--warmup 3] [--rounds 4] [--skip-step]

RN50 geometry (layers (3, 4, 6, 3), width 64, 224 px, 32 heads over 50 tokens) on synthetic weights.

(a) Forward: ``ClipResNet`` and, as the yardstick that exists on the parent commit, ``MocoResNet50`` (torchvision's
    ResNet-50 on the same GEMM kernel) on the same batch, alternating in one process: --rounds rounds of
    --forwards / --rounds forwards each after --warmup warm-ups, one HIP-event pair per forward; median, minimum and maximum
    in ms, images/s, and the TFLOP/s of the convolution GEMMs (2 M N K of every convolution's GEMM as launched, summed --
    the stem's K = 27 counts as the 28 the kernel multiplies -- over the median forward time: an end-to-end figure that
    charges im2col, pools and head to the GEMMs, not a kernel's rate).
(b) Shares: one further forward of each runner with a HIP-event pair around every launch, summed per kind: im2col (with the
    NCHW -> NHWC permute), pools, convolution GEMMs, head (token assembly, the three head GEMMs, attention).  At this batch
    every kernel runs for far longer than its launch takes to issue, so a pair brackets the kernel; the sum is printed next
    to the untimed forward to show what the bracketing itself adds.  ``conv_gemm_tflops_in_kernel`` is the same FLOP count
    over the GEMM kind's own time.
(c) One ``LoRATrainer`` step, encoder='text' (rank-4 q / k / v adapters on the 12 text blocks, dropout 0.25, 4 prompt
    tokens), on the cfg-2 counts: 256 images, 403 captions.  The image side is the frozen forward of (a).

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

RN50 = dict(layers=(3, 4, 6, 3), width=64, resolution=224, embed_dim=1024)
KINDS = {"clipfs_nchw_to_nhwc": "im2col", "clipfs_im2col_nhwc": "im2col", "clipfs_avgpool_nhwc": "pools",
         "clipfs_maxpool3x3s2_nhwc": "pools", "clipfs_global_avgpool_nhwc": "pools", "clipfs_attnpool_tokens": "head",
         "clipfs_attnpool_attend": "head", "clipfs_gemm_nt": "conv_gemm"}


def stats(xs, digits=3):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits), "max": round(max(xs), digits)}


def timed(fn, n):
    out = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


class Bracket:
    """Wraps the library's entry points for one forward: a HIP-event pair per launch, GEMM shapes noted."""

    def __init__(self, lib):
        self.lib, self.events, self.flops, self.in_head = lib, [], 0.0, False
        self.saved = {}

    def __enter__(self):
        for name in KINDS:
            fn = getattr(self.lib, name)
            self.saved[name] = fn
            setattr(self.lib, name, self._wrap(name, fn))
        return self

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(self.lib, name, fn)

    def _wrap(self, name, fn):
        def call(*args):
            kind = KINDS[name]
            if name == "clipfs_gemm_nt":
                g = args[0]._obj
                if self.in_head:
                    kind = "head"
                else:
                    self.flops += 2.0 * g.M * g.N * g.K
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*args)
            e1.record()
            self.events.append((kind, e0, e1))
            return rc
        return call

    def table(self):
        torch.cuda.synchronize()
        ms = {}
        for kind, e0, e1 in self.events:
            ms[kind] = ms.get(kind, 0.0) + e0.elapsed_time(e1)
        return ms, len(self.events)


def shares(lib, run, images):
    with Bracket(lib) as b:
        head = getattr(run, "head", None)
        if head is not None:
            def in_head(*a):
                b.in_head = True
                try:
                    return head(*a)
                finally:
                    b.in_head = False
            run.head = in_head
        try:
            run(images)
        finally:
            if head is not None:
                del run.head
        ms, launches = b.table()
    total = sum(ms.values())
    out = {k: {"ms": round(v, 3), "share": round(v / total, 4)} for k, v in sorted(ms.items())}
    out["sum_ms"], out["launches"] = round(total, 3), launches
    return out, b.flops, ms.get("conv_gemm", 0.0)


def forward_part(dev, args):
    from clipfs import _lib, resnet, synth
    clip_run = resnet.ClipResNet(resnet.synth_clip_resnet_state_dict(seed=7, **RN50), dev)
    moco_run = resnet.MocoResNet50(resnet.synth_resnet50_state_dict(seed=7), dev)
    images = synth.synth_images(args.batch, 224, seed=0).to(dev)
    runs = {"clip_rn50": clip_run, "moco_resnet50": moco_run}
    for r in runs.values():
        timed(lambda: r(images), args.warmup)
    per = max(1, -(-args.forwards // args.rounds))
    times = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, r in runs.items():
            times[k] += timed(lambda: r(images), per)
    out = {"batch": args.batch, "sample": f"{args.rounds} alternating rounds x {per} forwards per runner after {args.warmup} warm-ups"}
    for k, r in runs.items():
        table, flops, gemm_ms = shares(_lib.load(), r, images)
        med = statistics.median(times[k])
        out[k] = {"forward_ms": stats(times[k]), "images_per_s": round(1e3 * args.batch / med, 1),
                  "conv_gemm_gflop_per_forward": round(flops / 1e9, 2),
                  "conv_gemm_tflops_end_to_end": round(flops / med / 1e9, 2),
                  "conv_gemm_tflops_in_kernel": round(flops / gemm_ms / 1e9, 2) if gemm_ms else None,
                  "launch_kinds": table}
    a, b = out["clip_rn50"], out["moco_resnet50"]
    out["clip_over_moco_tflops_end_to_end"] = round(a["conv_gemm_tflops_end_to_end"] / b["conv_gemm_tflops_end_to_end"], 4)
    return out


def step_part(dev, args, batch=256, classes=403):
    import lora_train_vlp as L
    from clipfs import resnet, synth
    from jclip.model import build_model
    # RN50's text tower: width 512, 12 blocks, 8 heads, embedding 1024 (the vision fields of the config are not used)
    text = synth.ClipConfig("rn50-text", 1024, 224, 1, 64, 32, 77, 49408, 512, 12)
    sd = resnet.synth_clip_resnet_state_dict(seed=7, text=text, **RN50)
    model = build_model(sd, device=dev)
    a = types.SimpleNamespace(encoder="text", position="all", backbone="RN50", params=["q", "k", "v"], r=4, alpha=1,
                              dropout_rate=0.25)
    L.apply_lora(a, model)
    L.mark_only_lora_as_trainable(model)
    ctx = torch.nn.Parameter(model.token_embedding.weight.data[[5, 6, 7, 8]].clone())
    tr = L.LoRATrainer(model, prompt_ctx=ctx, shard_text=False)
    model.train()
    data = (synth.synth_images(batch, 224, seed=0).to(dev), synth.synth_captions(classes, 77, text.vocab_size, seed=1).to(dev),
            synth.synth_labels(batch, classes, seed=2).to(dev))
    timed(lambda: tr.step(*data, 1, batch), args.warmup)
    t = timed(lambda: tr.step(*data, 1, batch), args.steps)
    return {"images": batch, "captions": classes, "step_ms": stats(t), "steps": args.steps, "plan": tr.last_plan,
            "flat_floats": tr.flat.numel}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--forwards", type=int, default=24, help="timed forwards per runner (at least 20 for the record)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10, help="timed LoRATrainer steps of part (c)")
    ap.add_argument("--skip-step", action="store_true", help="parts (a) and (b) only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_clip_resnet.py needs an MI355X")
    dev = torch.device("cuda:0")
    out = {"rn50_forward": forward_part(dev, args)}
    if not args.skip_step:
        out["lora_text_step_rn50_256x403"] = step_part(dev, args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
