"""Times the fused transductive fit (csrc/transduct.hip, ``ops.transduct_fit``) against the same rule composed from what the
tree had before it: ``ops.gemm_nt`` in row chunks + ``torch.topk`` per chunk for the kNN affinity (the N x N similarities
pass through memory a chunk at a time), ``torch.log_softmax`` / ``torch.topk`` for the initial state, and per sweep an index
gather, elementwise launches and ``torch.softmax``, with ``z.T @ F`` for the class statistics.

Sizes: N 8192 and N 50000 at C 1000, d 512, k 3 (``--sizes``).  Fused and composed alternate in one process, warm; each
phase (kNN, init, one outer iteration) and the whole fit are timed with a pair of events on the stream, and medians over
``--calls`` calls are reported with min and max, the launch counts (the plan's for the fused side, the profiler's for both
where it is available), and the kNN launch's rate against the 157 TFLOP/s fp32 matrix peak (2 N^2 d flops: the full
matrix, the symmetry is not exploited).  ``python bench.py`` runs nothing of this.

    python scripts/bench_transduct.py [--calls 5] [--sizes 8192 50000] [--out FILE.json]
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

PEAK_TFLOPS = 157.3
ROW_CHUNK = 4096  # rows of F F^T the composed route holds at once: 4096 x 50000 fp32 = 0.8 GB


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


def clusters(C, n, d, dev, seed):
    """Class prototypes around a common direction, noisy features, noisier class features (the generator of
    tests/transduct_ref.py, on the device)."""
    gen = torch.Generator(dev).manual_seed(seed)
    unit = lambda x: torch.nn.functional.normalize(x, dim=-1)
    rn = lambda *s: torch.randn(*s, device=dev, generator=gen)
    proto = unit(unit(rn(1, d)) + 0.5 * unit(rn(C, d)))
    y = torch.randint(0, C, (n,), device=dev, generator=gen)
    F = unit(proto[y] + 1.0 / math.sqrt(d) * rn(n, d))
    T = unit(proto + 0.5 * unit(rn(C, d)))
    return F.contiguous(), T.contiguous(), y


class Composed:
    """The rule on torch and ``ops.gemm_nt``; the same phases as the fused stages."""

    def __init__(self, F, T, hp):
        self.F, self.T, self.hp = F, T, hp

    def knn(self):
        from clipfs import ops
        F, k = self.F, self.hp["k"]
        N = F.shape[0]
        ws, js = [], []
        for r0 in range(0, N, ROW_CHUNK):
            A = ops.gemm_nt(F[r0:r0 + ROW_CHUNK], F)
            rows = torch.arange(r0, min(N, r0 + ROW_CHUNK), device=F.device)
            A[rows - r0, rows] = float("-inf")
            w, j = torch.topk(A, k, dim=1)
            ws.append(w)
            js.append(j)
        self.w, self.nbr = torch.cat(ws), torch.cat(js)

    def init(self):
        from clipfs import ops
        F, hp = self.F, self.hp
        d = F.shape[1]
        self.logy = torch.log_softmax(ops.gemm_nt(F, self.T, alpha=hp["logit_scale"]), dim=1)
        self.z = self.logy.exp()
        sel = torch.topk(self.logy, hp["init_top"], dim=0).indices.T
        self.mu = F[sel].sum(dim=1) / hp["init_top"]
        self.var = torch.full((d,), 1.0 / d, device=F.device)
        self.Q = (F * F).sum(dim=0)

    def outer(self):
        from clipfs import ops
        F, hp = self.F, self.hp
        mup = (self.mu / self.var).contiguous()
        u = hp["lam"] * self.logy + ops.gemm_nt(F, mup, bias=(-0.5 * (self.mu * mup).sum(dim=1)).contiguous())
        z = self.z
        for _ in range(hp["inner"]):
            z = torch.softmax(u + (self.w[:, :, None] * z[self.nbr]).sum(dim=1), dim=1)
        n = z.sum(dim=0)
        G = z.T @ F
        mu = torch.where((n > hp["n_min"])[:, None], G / n[:, None], self.mu)
        var = (self.Q - 2 * (mu * G).sum(dim=0) + (n[:, None] * mu * mu).sum(dim=0)) / F.shape[0]
        self.z, self.mu, self.var = z, mu, var.clamp_min(hp["var_floor"])

    def fit(self):
        self.knn()
        self.init()
        for _ in range(self.hp["outer"]):
            self.outer()
        return self.z


def run(N, C, d, calls, dev):
    from clipfs import ops
    hp = dict(ops.TRANSDUCT_DEFAULTS)
    F, T, y = clusters(C, N, d, dev, seed=0)
    plan = ops.transduct_plan(N, C, d)
    bufs = ops.transduct_buffers(N, C, d, dev)
    res = {"N": N, "C": C, "d": d, "k": hp["k"], "fused_launches_plan": plan["launches"], "knn_chunks": plan["knn_chunks"],
           "knn_work_bytes": plan["knn_work_bytes"], "stat_splits": plan["stat_splits"]}
    comp = Composed(F, T, hp)
    composed_ok = True
    try:
        comp.fit()
    except RuntimeError as e:  # the composed route's chunks do not fit
        composed_ok = False
        res["composed_error"] = str(e).splitlines()[0][:200]
    fused_fit = lambda: ops.transduct_fit(F, T, buffers=bufs)
    fused_fit()
    torch.cuda.synchronize()
    if composed_ok:
        zc = comp.fit()
        zf = bufs["z"]
        res["max_abs_diff_z_fused_vs_composed"] = float((zf - zc).abs().max())
        res["labels_agree"] = float((zf.argmax(1) == zc.argmax(1)).float().mean())
        res["top1_zero_shot"] = float((bufs["zs_labels"].long() == y).float().mean())
        res["top1_transductive"] = float((bufs["labels"].long() == y).float().mean())
        res["neighbour_rows_equal"] = float((bufs["nbr"].long() == comp.nbr).all(dim=1).float().mean())
    # fused phases through the stage ops on the fit's own state
    logy, mu, mup = bufs["logy"], bufs["mu"].clone(), bufs["mup"].clone()
    st = ops.transduct_init(F, logy)
    work = torch.empty(plan["knn_work_bytes"] // 4, device=dev)

    def fused_outer():
        u, _ = ops.transduct_u(F, logy, mu, mup)
        z = bufs["z"]
        for _ in range(hp["inner"]):
            z = ops.transduct_z_step(u, bufs["nbr"], bufs["w"], z)
        ops.transduct_stats(F, z, mu, st["shot_n"], st["shot_G"], st["Q"])

    def fused_init():
        ops.transduct_logy(F, T)
        ops.transduct_init(F, logy)

    phases = {"knn": (lambda: ops.transduct_knn(F, hp["k"], work=work), comp.knn), "init": (fused_init, comp.init),
              "outer_iteration": (fused_outer, comp.outer), "fit": (fused_fit, comp.fit)}
    for name, (ff, cf) in phases.items():
        ff()
        tf, tc = [], []
        for _ in range(calls):
            tf.append(_time(ff))
            if composed_ok:
                tc.append(_time(cf))
        res[name] = {"fused": _q(tf)}
        if composed_ok:
            res[name]["composed"] = _q(tc)
            res[name]["composed_over_fused"] = round(statistics.median(tc) / statistics.median(tf), 2)
    t_knn = res["knn"]["fused"]["median_ms"] * 1e-3
    res["knn_tflops"] = round(2.0 * N * N * d / t_knn / 1e12, 2)
    res["knn_fraction_of_fp32_matrix_peak"] = round(res["knn_tflops"] / PEAK_TFLOPS, 3)
    res["fused_launches_profiled"] = _launches(fused_fit)
    if composed_ok:
        res["composed_launches_profiled"] = _launches(comp.fit)
    print(json.dumps({f"N{N}": res}), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[8192, 50000])
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "calls": args.calls, "row_chunk_of_the_composed_affinity": ROW_CHUNK}
    for N in args.sizes:
        out[f"N{N}"] = run(N, args.classes, args.width, args.calls, dev)
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
