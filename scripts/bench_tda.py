"""Times the training-free dynamic adapter (csrc/tda.hip, ``ops.tda_adapt``: one fused call per batch) against the
published per-sample form composed from what the tree had before it: per sample ``ops.gemm_nt`` for the zero-shot logits,
torch softmax / entropy, a host decision (one synchronisation), host-side queues (Python lists per class), and
``ops.cache_logits`` / ``ops.gemm_nt`` for the two cache terms.  Two geometries, B = 256 samples per measurement:

    imagenet  C = 1000, d = 512, Sp 3, Sn 2
    project   C = 403,  d = 512, Sp 3, Sn 2

Both sides start every measurement from the same warm caches (a stream of 1024 samples already adapted).  Fused and
per-sample alternate in one process, warm; each is timed with a pair of events on the stream and the medians over
``--calls`` calls (at least 20 fused, at least 5 of the slow loop) are reported with min and max, launches per 256 samples
for both (counted by the profiler where it is available, else the plan's count for the fused side and null), and, for
scale, the time of a ViT-B/32 image tower forward over 256 images.

    python scripts/bench_tda.py [--calls 20] [--geometry imagenet project] [--no-tower] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "jittor-clip-fewshot_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

GEOMETRIES = {"imagenet": dict(C=1000, d=512, B=256), "project": dict(C=403, d=512, B=256)}


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _q(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_max_ms": [round(min(xs), 4), round(max(xs), 4)], "calls": len(xs)}


def _launches(fn):
    """Kernel launches of one call of ``fn``, counted by the profiler; None where that is not available."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "emcpy" not in e.name
                and "emset" not in e.name)
        return n or None
    except Exception:  # noqa: BLE001 -- a measurement aid only
        return None


def clustered(C, n, d, dev, seed):
    """The clustered generator of tests/tda_ref.py on the device: cosines in a narrow band, as CLIP's are."""
    gen = torch.Generator(dev).manual_seed(seed)
    unit = lambda x: torch.nn.functional.normalize(x, dim=-1)
    u = unit(torch.randn(d, device=dev, generator=gen))
    g = torch.randn(C, d, device=dev, generator=gen) / math.sqrt(d)
    y = torch.randint(0, C, (n,), device=dev, generator=gen)
    a = 0.25 * torch.rand(n, device=dev, generator=gen)
    noise = torch.randn(n, d, device=dev, generator=gen) / math.sqrt(d)
    return unit(u + 0.35 * g).contiguous(), unit(u + 1.05 * a[:, None] * g[y] + 0.35 * noise).contiguous()


class PerSampleTDA:
    """The published one-image-at-a-time form on ops the tree already had: dictionaries of lists, a host decision per
    image.  Same rule as the fused call (same thresholds, the same tie rule through Python's stable ordering)."""

    def __init__(self, text, hp):
        self.text, self.hp = text, hp
        self.C = text.shape[0]
        self.pos, self.neg, self.t = {}, {}, 0

    def load(self, state):
        """Queues from a device state of ``ops.tda_new_state`` layout."""
        self.pos, self.neg = {}, {}
        self.t = int(state["counter"])
        for name, dst in (("pos", self.pos), ("neg", self.neg)):
            seq, ent = state[name + "_seq"].cpu(), state[name + "_ent"].cpu()
            for c, k in (seq >= 0).nonzero().tolist():
                item = [state[name + "_keys"][c, k].clone(), float(ent[c, k]), int(seq[c, k])]
                if name == "neg":
                    item.append(state["neg_mask"][c, k].float())
                dst.setdefault(c, []).append(item)

    @staticmethod
    def _offer(cache, pred, item, cap):
        q = cache.setdefault(pred, [])
        if len(q) < cap:
            q.append(item)
        else:
            w = max(range(len(q)), key=lambda k: (q[k][1], q[k][2]))
            if item[1] < q[w][1]:
                q[w] = item

    def step(self, f):
        from clipfs import ops
        hp = self.hp
        z = ops.gemm_nt(f, self.text, alpha=hp["logit_scale"])
        logp = torch.log_softmax(z, dim=1)
        p = logp.exp()
        H, pred = float(-(p * logp).sum()), int(z.argmax())  # the host decision: one synchronisation
        h = H / math.log2(self.C)
        self._offer(self.pos, pred, [f[0], H, self.t], hp["pos_cap"])
        if hp["ent_lo"] < h < hp["ent_hi"]:
            mask = ((p[0] > hp["mask_lo"]) & (p[0] < hp["mask_hi"])).float()
            self._offer(self.neg, pred, [f[0], H, self.t, mask], hp["neg_cap"])
        self.t += 1
        out = z
        if self.pos:
            classes = sorted(self.pos)
            keys = torch.stack([it[0] for c in classes for it in self.pos[c]])
            counts = torch.zeros(self.C + 1, dtype=torch.int32)
            for c in classes:
                counts[c + 1] = len(self.pos[c])
            off = counts.cumsum(0).to(torch.int32).to(f.device)
            out = ops.cache_logits(f, keys, off, z, hp["pos_alpha"], hp["pos_beta"])
        if self.neg:
            items = [it for q in self.neg.values() for it in q]
            keys = torch.stack([it[0] for it in items])
            masks = torch.stack([it[3] for it in items])
            E = torch.exp(-hp["neg_beta"] * (1.0 - ops.gemm_nt(f, keys)))
            n = keys.shape[0]  # any count: the strided VALU product (gemm_nt needs a reduction length that is a multiple of 4)
            out = out - ops.matmul_small(E, masks, 1, self.C, n, n, 1, self.C, 1, alpha=hp["neg_alpha"])
        return out

    def adapt(self, F):
        return torch.cat([self.step(F[b:b + 1]) for b in range(F.shape[0])])


def run(name, g, calls, dev):
    from clipfs import ops
    C, d, B = g["C"], g["d"], g["B"]
    hp = dict(ops.TDA_DEFAULTS)
    text, stream = clustered(C, 1024 + B, d, dev, seed=0)
    warm = ops.tda_new_state(C, d, hp["pos_cap"], hp["neg_cap"], dev)
    ops.tda_adapt(stream[:1024], text, warm)
    F = stream[1024:].contiguous()
    state = {k: v.clone() for k, v in warm.items()}
    record = ops.tda_new_record(C, B, hp["pos_cap"], hp["neg_cap"], dev)
    out = torch.empty(B, C, device=dev)
    loop = PerSampleTDA(text, hp)

    def fused():
        for k, v in warm.items():  # both sides start from the warm caches; the copies are part of neither timing
            state[k].copy_(v)
        return _time(lambda: ops.tda_adapt(F, text, state, out=out, record=record))

    def composed():
        loop.load(warm)
        torch.cuda.synchronize()
        return _time(lambda: loop.adapt(F))

    fused(), composed(), fused()
    got = out.clone()
    loop.load(warm)
    want = loop.adapt(F)
    res = {"geometry": g, "max_abs_diff_fused_vs_per_sample": float((got - want).abs().max()),
           "top1_agree": float((got.argmax(1) == want.argmax(1)).float().mean())}
    n_loop = max(5, min(calls, 8))
    tf, tc = [], []
    for k in range(max(20, calls)):
        tf.append(fused())
        if k < n_loop:
            tc.append(composed())
    res["fused"] = _q(tf)
    res["per_sample"] = _q(tc)
    res["per_sample_over_fused"] = round(statistics.median(tc) / statistics.median(tf), 1)
    plan = ops.tda_plan(C, d, B)
    res["fused_launches_plan"] = plan["launches"]
    res["fused_lds_bytes"] = plan["lds_bytes"]
    res["fused_launches_profiled"] = _launches(lambda: ops.tda_adapt(F, text, state, out=out, record=record))
    loop.load(warm)
    res["per_sample_launches_profiled"] = _launches(lambda: loop.adapt(F))
    res["inserted"] = {"pos": int((record["pos_slot"] >= 0).sum()), "neg": int((record["neg_slot"] >= 0).sum())}
    print(json.dumps({name: res}), flush=True)
    return res


def tower(calls, dev):
    from clipfs import synth
    from jclip.model import build_model
    model = build_model(synth.synth_state_dict(synth.VIT_B32, seed=1), device=dev)
    images = synth.synth_images(256, 224, seed=3).to(dev)
    with torch.no_grad():
        for _ in range(3):
            model.encode_image(images)
        ts = [_time(lambda: model.encode_image(images)) for _ in range(max(10, calls))]
    res = {"model": "ViT-B/32 (synthetic weights)", "images": 256, **_q(ts)}
    print(json.dumps({"tower_forward": res}), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--geometry", nargs="+", default=list(GEOMETRIES), choices=list(GEOMETRIES))
    ap.add_argument("--no-tower", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "calls": max(20, args.calls)}

    def save():
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(out, fh, indent=1)

    for name in args.geometry:
        out[name] = run(name, GEOMETRIES[name], args.calls, dev)
        save()
    if not args.no_tower:
        out["tower_forward"] = tower(args.calls, dev)
        save()


if __name__ == "__main__":
    main()
