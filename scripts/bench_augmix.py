"""AugMix view generation on the device (csrc/augmix.hip) against the plain crops it replaces and the tower pass it feeds.

    python scripts/bench_augmix.py [--images 8] [--views 63] [--reps 7] [--no-tower]

Workload: G images of 375 x 500, 1 + views views each, S = 224, width 3, severity 1 and severity 3.  Prints one JSON line:
  view_groups_ms      device time of one ``augmix.view_groups`` call (events around the call: recipe upload + 3 launches),
                      median of --reps, the arms alternating (severity 1, severity 3, crop_batch, tower) within every rep;
  launch_ms           device time per launch (base, chains, mix) from the profiler's kernel records, median over the calls
                      it saw (null when the profiler reports no kernels);
  host_sample_ms      host time to sample the crop records and the recipe; host_enqueue_ms: host time of the
                      ``augmix_batch`` call itself (packing, pinning and uploading the tables, validation, three launches);
  crop_batch_ms       ``data.crop_batch`` on the same records: plain crops are what TPT gets without AugMix, the floor;
  tower_ms            the ViT-B/32 image tower forward (fp32) over the same G (1 + views) views: the work the views feed.
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jittor-clip-fewshot_amd"))
sys.path.insert(0, ROOT)


def synth_image(h, w, seed):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack([np.sin(xx / 31.0), np.cos(yy / 17.0), np.sin((xx + yy) / 23.0)], -1) * 100 + 128
    return np.clip(base + rng.randint(-20, 20, (h, w, 3)), 0, 255).astype(np.uint8)


def event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def launch_times(fn, calls=3):
    """{launch: median device ms} of the three kernels over ``calls`` calls, from the profiler's kernel records."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        seen = {"base": [], "chains": [], "mix": []}
        names = {"augmix_base_kernel": "base", "augmix_chain_kernel": "chains", "augmix_mix_kernel": "mix"}
        for ev in prof.events():
            for key, launch in names.items():
                if key in ev.name and getattr(ev, "device_time", 0) > 0:
                    seen[launch].append(ev.device_time / 1e3)
        return {k: (round(float(np.median(v)), 4) if v else None) for k, v in seen.items()}
    except Exception as e:  # the profiler is a convenience here, not the measurement
        return {"base": None, "chains": None, "mix": None, "error": repr(e)[:200]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--views", type=int, default=63)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-tower", action="store_true")
    args = ap.parse_args()

    import torch
    from clipfs import augmix, data
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    G, V, S, width = args.images, 1 + args.views, 224, 3
    pool = data.ImagePool.from_arrays([synth_image(375, 500, k) for k in range(G)], list(range(G)), device=dev)
    idx = list(range(G))
    out = torch.empty(G, V, 3, S, S, device=dev)
    res = {"images": G, "views": V, "size": S, "width": width, "reps": args.reps, "plan": augmix._lib.augmix_plan(G * V, S, width)}

    t0 = time.perf_counter()
    recs, plain = augmix.group_records(pool, idx, args.views, size=S, seed=0)
    recipes = {sev: augmix.sample_recipes(G * V, S, width=width, severity=sev, seed=0, plain=plain) for sev in (1, 3)}
    res["host_sample_ms"] = round((time.perf_counter() - t0) * 1e3 / 2, 3)  # records once, two recipes: per recipe, roughly
    res["ops_per_recipe"] = {sev: int(r.depth.sum()) for sev, r in recipes.items()}
    res["affine_ops"] = {sev: int(sum((r.ops[v, i, s, 0] == augmix.AFFINE) for v in range(G * V) for i in range(width)
                                      for s in range(r.depth[v, i]))) for sev, r in recipes.items()}

    flat = out.view(G * V, 3, S, S)
    arms = {f"severity{sev}": (lambda r=recipes[sev]: augmix.augmix_batch(pool, recs, r, S, out=flat)) for sev in (1, 3)}
    arms["crop_batch"] = lambda: data.crop_batch(pool, recs, S, flat)
    if not args.no_tower:
        import bench
        bargs = types.SimpleNamespace(dropout=0.0, no_shard_text=False, serial_towers=False, trim_text=False, precision="fp32",
                                      model="b32")
        model, _, _ = bench.build_trainer(dev, bargs)
        model.eval()

        def tower():
            with torch.no_grad():
                model.engine.vit_forward(flat, False, 0)
        arms["tower"] = tower

    for fn in arms.values():  # warm: allocations, LDS attributes, GEMM plans
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(args.reps):  # the arms alternate so that clock drift hits all of them
        for k, fn in arms.items():
            times[k].append(event_ms(fn))
    med = {k: round(float(np.median(v)), 4) for k, v in times.items()}
    res["view_groups_ms"] = {"severity1": med["severity1"], "severity3": med["severity3"]}
    res["crop_batch_ms"] = med["crop_batch"]
    res["tower_ms"] = med.get("tower")
    res["all_ms"] = {k: [round(x, 4) for x in v] for k, v in times.items()}
    host = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        arms["severity3"]()
        host.append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    res["host_enqueue_ms"] = round(float(np.median(host)), 3)
    res["launch_ms"] = {k: launch_times(arms[k]) for k in ("severity1", "severity3")}
    if res["tower_ms"]:
        res["generation_over_tower"] = {k: round(v / res["tower_ms"], 4) for k, v in res["view_groups_ms"].items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
