"""Packed (live-row) text backward in the fp16 storage mode: what it saves at cfg-5's geometry.

    python scripts/bench_pack_f16.py [--steps 10] [--warmup 3] [--rounds 4] [--batch 128] [--classes 403]

bench.py's cfg-5 trainer (ViT-L/14, rank-16 q/k/v adapters, LoRA dropout 0.25, prompt ctx, precision fp16; 128 images +
403 captions) on ONE model: rounds of --steps training steps with ``Engine.pack_text_backward`` on, then off, alternating
in one process after --warmup warm-ups of each arm; per-step HIP-event times.  The forward is the same in both arms
(clipfs_tower_pack_fwd_mode is 0 in fp16 mode), so the difference is the text backward's.  Each arm is measured twice:
the two towers on two streams (bench.py's default) and one after the other (``overlap_towers = False``), where the
step-time difference is the text backward's own kernel time.

Prints one JSON object: median / minimum / maximum per arm, the ratio of the medians, and the library's decision
(clipfs_tower_pack_mode, R of M rows) for the geometry."""
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


def summary(t):
    return {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--classes", type=int, default=403)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pack_f16.py needs an MI355X")
    import bench
    from clipfs import synth
    dev = torch.device("cuda:0")
    a = types.SimpleNamespace(model="l14", dropout=0.25, no_shard_text=False, serial_towers=False, trim_text=False,
                              precision="fp16")
    model, tr, cfg = bench.build_trainer(dev, a)
    eng = model.engine
    data = (synth.synth_images(args.batch, 224, seed=0).to(dev),
            synth.synth_captions(args.classes, 77, cfg.vocab_size, seed=1).to(dev),
            synth.synth_labels(args.batch, 374, seed=2).to(dev))
    out = {"shapes": f"ViT-L/14 fp16, {args.batch} images + {args.classes} captions, q/k/v adapters r = 16, dropout 0.25, "
                     "prompt ctx",
           "sample": f"{args.rounds} alternating rounds x {args.steps} steps per arm after {args.warmup} warm-ups"}
    for label, overlap in (("two_streams", True), ("serial_towers", False)):
        tr.overlap_towers = overlap
        for pack in (True, False):
            eng.pack_text_backward = pack
            time_steps(tr, data, args.batch, args.warmup)
        times = {True: [], False: []}
        for _ in range(args.rounds):
            for pack in (True, False):
                eng.pack_text_backward = pack
                times[pack] += time_steps(tr, data, args.batch, args.steps)
        res = {"packed": summary(times[True]), "dense": summary(times[False])}
        res["packed_over_dense_median"] = round(res["packed"]["median_ms"] / res["dense"]["median_ms"], 4)
        res["dense_minus_packed_median_ms"] = round(res["dense"]["median_ms"] - res["packed"]["median_ms"], 3)
        out[label] = res
    eng.pack_text_backward = True
    ids, seq = eng._effective_ids(data[1])
    _, R = eng._pack_plan(ids)
    out["pack_mode"] = int(eng.txt.pack_mode(ids.shape[0], R, 1, seq, tr.last_plan["text"]))
    out["live_rows"], out["dense_rows"] = R, ids.shape[0] * seq
    print(json.dumps(out))


if __name__ == "__main__":
    main()
