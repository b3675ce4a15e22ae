"""Training-batch generation: GPU crop kernel (csrc/crops.hip) and TrainLoader against the reference's CPU/PIL path.

    python scripts/bench_train_loader.py [--steps 20] [--cpu-images 1024] [--no-cpu] [--no-step]

Prints one JSON line:
  (a) kernel_ms       one 256-view clipfs_crop_batch launch (CLIP-normalised output; and both outputs) from a pool of
                      1 495 synthetic images: 70 % 500x375 / 375x500, 25 % 1024x768 / 768x1024, 5 % 3000x2000
                      (the few-shot train split's size), records of RandomResizedCrop(224, scale=(0.05, 1)) + flip;
  (b) step_ms         the cfg-2 LoRATrainer step (bench.py's model, 256 images, 403 captions) fed by TrainLoader with
                      prefetch, against the same step on a fixed device tensor;
  (c) cpu_images_s    the reference's CPU path for the same transform (PIL decode of a JPEG, RandomResizedCrop, flip,
                      ImageNormalize, ToTensor) in a 16-process pool, images/s.
"""
import argparse
import io
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jittor-clip-fewshot_amd"))
sys.path.insert(0, ROOT)

N_POOL = 1495
MIX = ((0.35, (375, 500)), (0.35, (500, 375)), (0.125, (768, 1024)), (0.125, (1024, 768)), (0.05, (2000, 3000)))


def pool_sizes(n=N_POOL, seed=0):
    rng = np.random.RandomState(seed)
    p = np.array([m[0] for m in MIX])
    return [MIX[k][1] for k in rng.choice(len(MIX), size=n, p=p / p.sum())]


def synth_image(h, w, seed):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack([np.sin(xx / 31.0), np.cos(yy / 17.0), np.sin((xx + yy) / 23.0)], -1) * 100 + 128
    return np.clip(base + rng.randint(-20, 20, (h, w, 3)), 0, 255).astype(np.uint8)


# ---------------------------------------------------------------------------------------------- (c) CPU / PIL path
_JPEGS = None


def _cpu_init(jpegs):
    global _JPEGS
    _JPEGS = jpegs


def _cpu_one(i):
    """lora_train_vlp.py:1203-1208 train_tranform1 on one image: decode, RandomResizedCrop(224, (0.05, 1)),
    RandomHorizontalFlip, ImageNormalize, ToTensor."""
    from PIL import Image
    from clipfs.views import CLIP_MEAN, CLIP_STD, sample_crop
    rng = np.random.RandomState(i)
    im = Image.open(io.BytesIO(_JPEGS[i % len(_JPEGS)])).convert("RGB")
    top, left, h, w = sample_crop(im.width, im.height, (0.05, 1.0), (3 / 4, 4 / 3), rng)
    im = im.crop((left, top, left + w, top + h)).resize((224, 224), Image.BILINEAR)
    if rng.random_sample() < 0.5:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    a = np.asarray(im, dtype=np.float32)
    a = (a - np.float32(CLIP_MEAN) * 255) * ((1 / 255) / np.float32(CLIP_STD))
    return float(a.transpose(2, 0, 1).sum())


def cpu_rate(n_images, procs=16):
    import multiprocessing as mp
    from PIL import Image
    jpegs = []
    for k, (h, w) in enumerate(pool_sizes(64, seed=1)):
        buf = io.BytesIO()
        Image.fromarray(synth_image(h, w, k)).save(buf, format="JPEG", quality=90)
        jpegs.append(buf.getvalue())
    ctx = mp.get_context("spawn")  # no fork of a process that may hold a GPU context
    with ctx.Pool(procs, initializer=_cpu_init, initargs=(jpegs,)) as pool:
        pool.map(_cpu_one, range(procs * 4), chunksize=4)  # warm the workers
        t0 = time.perf_counter()
        pool.map(_cpu_one, range(n_images), chunksize=8)
        dt = time.perf_counter() - t0
    return n_images / dt


# ---------------------------------------------------------------------------------------------- (a), (b) GPU
def build_pool(dev):
    import torch
    from clipfs import data
    sizes = pool_sizes()
    distinct = {s: synth_image(s[0], s[1], k) for k, s in enumerate(sorted(set(sizes)))}
    # every entry is its own copy in the pool; content repeats per size, which the kernel does not care about
    arrays = [torch.from_numpy(distinct[s]) for s in sizes]
    return data.ImagePool.from_arrays(arrays, [i % 374 for i in range(len(sizes))], device=dev)


def time_ms(fn, reps, warm=3):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--cpu-images", type=int, default=1024)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    res = {"pool_images": N_POOL, "mix": {f"{h}x{w}": f for f, (h, w) in MIX}}
    if not args.no_cpu:  # first, before this process opens the GPU
        res["cpu_procs"] = 16
        res["cpu_images_s"] = round(cpu_rate(args.cpu_images), 1)

    import torch
    from clipfs import data
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    t0 = time.perf_counter()
    pool = build_pool(dev)
    torch.cuda.synchronize()
    res["pool_build_s"] = round(time.perf_counter() - t0, 2)
    res["pool_gb"] = round(pool.data.numel() / 1e9, 3)
    ld = data.TrainLoader(pool, batch_size=256, seed=0, outputs=("clip", "raw"))
    recs = ld.epoch_records(0)[:256]
    norm = torch.empty(256, 3, 224, 224, device=dev)
    raw = torch.empty_like(norm)
    res["kernel_ms"], _ = time_ms(lambda: data.crop_batch(pool, recs, 224, norm), 30)
    res["kernel_both_outputs_ms"], _ = time_ms(lambda: data.crop_batch(pool, recs, 224, norm, raw), 30)
    res["max_taps_in_batch"] = int(max(max(data.crop_taps(0, r[4], 224), data.crop_taps(0, r[3], 224)) for r in recs))

    if not args.no_step:
        import bench
        from clipfs import synth
        bargs = types.SimpleNamespace(dropout=0.25, no_shard_text=False, serial_towers=False, trim_text=False,
                                      precision="fp32", model="b32")
        model, tr, cfg = bench.build_trainer(dev, bargs)
        captions = synth.synth_captions(403, 77, cfg.vocab_size, seed=1).to(dev)
        images = synth.synth_images(256, 224, seed=0).to(dev)
        labels = synth.synth_labels(256, 374, seed=2).to(dev)

        def run_fixed(n):
            for _ in range(n):
                tr.step(images, captions, labels)

        loader = data.TrainLoader(pool, batch_size=256, seed=0, drop_last=True, prefetch=True)

        def run_loader(n):
            done = 0
            while done < n:
                for img, _, tgt, _ in loader:
                    tr.step(img, captions, tgt)
                    done += 1
                    if done == n:
                        break

        def per_step(fn, n):
            fn(3)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(n)
            b.record()
            b.synchronize()
            return a.elapsed_time(b) / n

        # alternate the two legs so that clock drift hits both
        fixed, fed = [], []
        for _ in range(3):
            fixed.append(per_step(run_fixed, args.steps))
            fed.append(per_step(run_loader, args.steps))
        res["step_fixed_ms"] = round(float(np.median(fixed)), 3)
        res["step_loader_ms"] = round(float(np.median(fed)), 3)
        res["step_fixed_ms_all"] = [round(v, 3) for v in fixed]
        res["step_loader_ms_all"] = [round(v, 3) for v in fed]
        res["loader_overhead_pct"] = round(100 * (res["step_loader_ms"] / res["step_fixed_ms"] - 1), 2)
    res["kernel_ms"] = round(res["kernel_ms"], 4)
    res["kernel_both_outputs_ms"] = round(res["kernel_both_outputs_ms"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
