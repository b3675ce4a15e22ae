#!/usr/bin/env python
"""Merged-weight evaluation on the MI355X: what a merge costs and what the evaluation forward gains.

1. Merge time per tower: the clipfs_lora_merge launch alone (device events around repeated launches of one uploaded
   table), beside its byte floor = (bytes read + bytes written) / 6.3 TB/s, the chip's measured float4 copy rate, and the
   wall time of ``tower.merge()`` (allocation, table upload and launch, host-synchronised).  ViT-B/32 with q k v at r 4
   and ViT-L/14 with all six projections at r 16, in each plane format.
2. Evaluation forward, merged against the adapter path: encode_image of 256 images + encode_text of 403 captions
   (cfg-2's shapes), eval mode, no grad.  Two models with the same weights, one merged, called alternately in one
   process; medians of device-event times.  q k v r 4, and q k v c_fc c_proj r 4 (where the live-row text forward and the
   one-row last block return); for the second also the fp16 storage mode, which has no adapter arm.

Synthetic weights (clipfs.synth): times do not depend on the values.  Prints one JSON line per figure; --out also writes
them to a file.  Needs the GPU: there is no CPU path."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jittor-clip-fewshot_amd"))

COPY_RATE = 6.3e12  # bytes / s, float4 copy
ATTN = {"q": "q_proj", "k": "k_proj", "v": "v_proj", "o": "proj"}
LINES = []


def emit(**kw):
    line = json.dumps(kw)
    LINES.append(line)
    print(line, flush=True)


def build(cfg, backbone, params, r, dev, seed=1234):
    import lora_train_vlp as L
    from clipfs import synth
    from jclip.model import build_model
    model = build_model(synth.synth_state_dict(cfg, seed=seed), device=dev)
    args = types.SimpleNamespace(encoder="both", position="all", backbone=backbone, params=list(params), r=r, alpha=1,
                                 dropout_rate=0.25)
    layers = L.apply_lora(args, model)
    rng = np.random.RandomState(5)
    with torch.no_grad():
        for layer in layers:
            for tok in params:
                m = getattr(layer, ATTN.get(tok, tok))
                m.w_lora_B.copy_(torch.from_numpy((rng.standard_normal(tuple(m.w_lora_B.shape)) * 0.02).astype(np.float32)))
    return model.eval()


def events_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def merge_times(name, model, reps):
    from clipfs import _lib, ops
    eng = model.engine
    lib = _lib.load()
    for tname, tower in (("text", eng.txt), ("vision", eng.vis)):
        jobs, r, scale = tower._adapted()
        for mode, fmt in ops.PLANE_FORMATS.items():
            table = (_lib.MergeJob * len(jobs))()
            keep, tile0, rd, wr = [], 0, 0, 0
            for rec, (_, _, w, a, b, nseg, mask) in zip(table, jobs):
                out = torch.empty_like(w)
                planes = ops.empty_planes(out, fmt)
                keep.append((out, planes))
                n, k = w.shape
                rec.w, rec.a, rec.b, rec.out = w.data_ptr(), a.data_ptr(), b.data_ptr(), out.data_ptr()
                rec.planes = None if planes is None else planes.data_ptr()
                rec.n, rec.k, rec.nseg, rec.seg_mask, rec.tile0 = n, k, nseg, mask, tile0
                tile0 += _lib.merge_job_tiles(n, k, nseg)
                rd += 4 * (n * k + a.numel() + b.numel())
                wr += 4 * n * k + (0 if planes is None else planes.numel() * planes.element_size())
            dev_table = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(model.device)
            stream = torch.cuda.current_stream().cuda_stream

            def launch():
                _lib.check(lib.clipfs_lora_merge(table, dev_table.data_ptr(), len(jobs), C.sizeof(_lib.MergeJob), r, scale, fmt,
                                                 stream), "lora_merge")

            ms = events_ms(launch, reps)
            tower.precision = mode
            wall = []
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tower.merge()
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
            tower.unmerge()
            tower.precision = "fp32"
            del keep
            emit(what="merge", model=name, tower=tname, planes=mode, jobs=len(jobs), tiles=tile0, r=r,
                 bytes_read=rd, bytes_written=wr, floor_us=round((rd + wr) / COPY_RATE * 1e6, 2),
                 kernel_us_median=round(statistics.median(ms) * 1e3, 2), kernel_us_min=round(min(ms) * 1e3, 2),
                 merge_call_wall_ms_median=round(statistics.median(wall), 3))


def eval_forward(name, adapter, merged, img, cap, reps, fp16=False):
    import lora_train_vlp as L

    def fwd(m):
        def f():
            with torch.no_grad():
                m.encode_image(img)
                m.encode_text(cap)
        return f

    L.merge_lora(merged)
    fa, fm = fwd(adapter), fwd(merged)
    for f in (fa, fm):
        events_ms(f, 1, warmup=3)
    ta, tm = [], []
    for _ in range(reps):  # alternate the arms
        ta += events_ms(fa, 1, warmup=0)
        tm += events_ms(fm, 1, warmup=0)
    with torch.no_grad():
        rel = ((merged.encode_text(cap) - adapter.encode_text(cap)).norm() / adapter.encode_text(cap).norm()).item()
    emit(what="eval_forward", model=name, images=img.shape[0], captions=cap.shape[0], precision="fp32",
         adapter_ms_median=round(statistics.median(ta), 3), adapter_ms_min=round(min(ta), 3), adapter_ms_max=round(max(ta), 3),
         merged_ms_median=round(statistics.median(tm), 3), merged_ms_min=round(min(tm), 3), merged_ms_max=round(max(tm), 3),
         text_feature_rel_diff=rel)
    if fp16:
        merged.engine.precision = "fp16"
        L.merge_lora(merged)
        t16 = events_ms(fm, reps, warmup=3)
        merged.engine.precision = "fp32"
        emit(what="eval_forward", model=name, images=img.shape[0], captions=cap.shape[0], precision="fp16",
             merged_ms_median=round(statistics.median(t16), 3), merged_ms_min=round(min(t16), 3), merged_ms_max=round(max(t16), 3))
    L.unmerge_lora(merged)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default="")
    ap.add_argument("--skip-l14", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_merged_eval needs the GPU: there is no CPU path")
    from clipfs import synth
    dev = torch.device("cuda:0")
    img = synth.synth_images(256, 224, seed=0).to(dev)
    cap = synth.synth_captions(403, 77, synth.VIT_B32.vocab_size, seed=1).to(dev)

    qkv = ("q", "k", "v")
    b32 = build(synth.VIT_B32, "ViT-B/32", qkv, 4, dev)
    merge_times("ViT-B/32 q k v r4", b32, a.reps)
    eval_forward("ViT-B/32 q k v r4", b32, build(synth.VIT_B32, "ViT-B/32", qkv, 4, dev), img, cap, a.reps)
    del b32
    five = qkv + ("c_fc", "c_proj")
    eval_forward("ViT-B/32 q k v c_fc c_proj r4", build(synth.VIT_B32, "ViT-B/32", five, 4, dev),
                 build(synth.VIT_B32, "ViT-B/32", five, 4, dev), img, cap, a.reps, fp16=True)
    if not a.skip_l14:
        torch.cuda.empty_cache()
        merge_times("ViT-L/14 all six r16", build(synth.VIT_L14, "ViT-L/14", qkv + ("o", "c_fc", "c_proj"), 16, dev), a.reps)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
