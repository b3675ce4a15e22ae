"""Times the GDA head (csrc/gda.hip on csrc/spd.hip; ``ops.gda_fit``, ``ops.gda_search``, ``ops.spd_factor``,
``ops.spd_solve``) against the same rule composed in torch on the device: ``index_add_`` class means, ``X.T @ X``,
``torch.linalg.cholesky`` + ``torch.cholesky_solve``, and the published ``torch.linalg.pinv`` form; the search as one
``argmax`` per grid cell on a ``g`` formed once.

Shapes: the fit at (C 1000, d 512, 16 shots), (C 1000, d 1024, 16 shots) and (C 403, d 512, 4 shots); the search at
B 8192 on the first; factor and solve alone at each d.  Both routes alternate in one process, warm; every timing is a
pair of events on the stream, medians over ``--calls`` calls with min and max, the plan's launch counts, and the
profiler's where it is available.  If this torch build has no device ``linalg`` the yardstick runs on the CPU and every
such number is labelled ``cpu``.  ``python bench.py`` runs nothing of this.

    python scripts/bench_gda.py [--calls 7] [--out profiles/gda/bench_gda.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "jittor-clip-fewshot_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

SHAPES = ((1000, 512, 16), (1000, 1024, 16), (403, 512, 4))
SEARCH_ROWS = 8192


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _time_cpu(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


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


def shots(C, d, per_class, dev, seed):
    gen = torch.Generator(dev).manual_seed(seed)
    unit = lambda x: torch.nn.functional.normalize(x, dim=-1)
    rn = lambda *s: torch.randn(*s, device=dev, generator=gen)
    centres = unit(rn(C, d))
    labels = torch.arange(C, device=dev).repeat_interleave(per_class)
    S = unit(centres[labels] + rn(labels.numel(), d) / d ** 0.5).contiguous()
    offsets = (torch.arange(C + 1, device=dev) * per_class).to(torch.int32)
    return S, labels, offsets, centres


class Composed:
    """The rule on torch; ``dev``: where its linear algebra runs."""

    def __init__(self, S, labels, C, dev):
        self.S, self.labels, self.C = S.to(dev), labels.to(dev), C
        self.counts = torch.bincount(self.labels, minlength=C).float()

    def gram(self):
        S, C = self.S, self.C
        M, d = S.shape
        self.mu = torch.zeros(C, d, device=S.device).index_add_(0, self.labels, S) / self.counts[:, None]
        X = S - self.mu[self.labels]
        G = X.T @ X
        self.A = G + torch.trace(G) / (M - 1) * torch.eye(d, device=S.device)

    def factor(self):
        self.L = torch.linalg.cholesky(self.A)

    def solve(self):
        d = self.S.shape[1]
        self.W = (d * torch.cholesky_solve(self.mu.T.contiguous(), self.L)).T.contiguous()

    def bias(self):
        self.b = -torch.log(torch.tensor(float(self.C), device=self.S.device)) - 0.5 * (self.mu * self.W).sum(1)

    def fit(self):
        self.gram()
        self.factor()
        self.solve()
        self.bias()

    def fit_pinv(self):
        self.gram()
        self.W = (self.S.shape[1] * (torch.linalg.pinv(self.A) @ self.mu.T)).T.contiguous()
        self.bias()


def device_linalg_works(dev):
    try:
        A = torch.eye(8, device=dev) * 2
        L = torch.linalg.cholesky(A)
        torch.cholesky_solve(torch.ones(8, 2, device=dev), L)
        torch.linalg.pinv(A)
        torch.cuda.synchronize()
        return True, None
    except Exception as e:  # noqa: BLE001
        return False, str(e).splitlines()[0][:200]


def _alternate(res, name, fused, composed, calls, timer_c=_time):
    fused()
    composed()
    tf, tc = [], []
    for _ in range(calls):
        tf.append(_time(fused))
        tc.append(timer_c(composed))
    res[name] = {"fused": _q(tf), "composed": _q(tc),
                 "composed_over_fused": round(statistics.median(tc) / statistics.median(tf), 3)}


def run(C, d, per_class, calls, dev, on_device):
    from clipfs import ops
    S, labels, offsets, centres = shots(C, d, per_class, dev, seed=0)
    M = S.shape[0]
    host = offsets.cpu()
    plan, sp = ops.gda_plan(M, C, d), ops.spd_plan(d, C)
    res = {"C": C, "d": d, "shots_per_class": per_class, "M": M, "fit_launches_plan": plan["launches"],
           "factor_launches_plan": sp["factor_launches"], "solve_launches_plan": sp["solve_launches"],
           "solve_workgroups": sp["solve_grid"], "lds_bytes": plan["lds_bytes"],
           "yardstick_device": "gpu" if on_device else "cpu"}
    cdev = dev if on_device else torch.device("cpu")
    timer = _time if on_device else _time_cpu
    comp = Composed(S, labels, C, cdev)
    bufs = ops.gda_buffers(M, C, d, dev)
    fused_fit = lambda: ops.gda_fit(S, offsets, offsets_host=host, buffers=bufs)
    fused_fit()
    comp.fit()
    torch.cuda.synchronize()
    res["info"] = int(bufs["info"].item())
    Wc = comp.W.to(dev)
    res["max_rel_diff_W_fused_vs_composed"] = float((bufs["W"] - Wc).abs().max() / Wc.abs().max())
    res["max_abs_diff_b_fused_vs_composed"] = float((bufs["b"] - comp.b.to(dev)).abs().max())
    _alternate(res, "fit", fused_fit, comp.fit, calls, timer)
    _alternate(res, "fit_vs_pinv_form", fused_fit, comp.fit_pinv, calls, timer)
    # where the time goes: the stages alone, on the fit's own buffers
    gram = bufs["gram"].clone()
    stages = {
        "stats": lambda: ops.gda_stats(S, offsets, offsets_host=host),
        "gram": lambda: ops.gemm_nt(bufs["xt"], bufs["xt"], split_k=False),
        "shrink": lambda: ops.gda_shrink(gram.clone(), M),
        "bias": lambda: ops.gda_bias(bufs["mu"], bufs["W"], offsets, M, offsets_host=host),
    }
    for name, fn in stages.items():
        fn()
        res["stage_" + name] = _q([_time(fn) for _ in range(calls)])
    chol = torch.empty_like(gram)
    _alternate(res, "factor", lambda: ops.spd_factor(bufs["gram"], out=chol), comp.factor, calls, timer)
    W = torch.empty_like(bufs["W"])
    _alternate(res, "solve", lambda: ops.spd_solve(bufs["chol"], bufs["mu"], alpha=float(d), out=W), comp.solve, calls, timer)
    res["fit_launches_profiled"] = _launches(fused_fit)
    if on_device:
        res["composed_fit_launches_profiled"] = _launches(comp.fit)
    return res, (bufs, centres)


def run_search(C, d, state, calls, dev):
    from clipfs import ops
    bufs, centres = state
    gen = torch.Generator(dev).manual_seed(1)
    target = torch.randint(0, C, (SEARCH_ROWS,), device=dev, generator=gen)
    F = torch.nn.functional.normalize(centres[target] + torch.randn(SEARCH_ROWS, d, device=dev, generator=gen) / d ** 0.5, dim=-1)
    F = F.contiguous()
    base = ops.gemm_nt(F, torch.nn.functional.normalize(centres, dim=-1).contiguous(), alpha=100.0)
    alphas = torch.tensor(ops.GDA_DEFAULT_ALPHAS, device=dev)
    W, b = bufs["W"], bufs["b"]

    def fused():
        g = ops.gemm_nt(F, W, bias=b, split_k=False)
        return ops.gda_search(g, base, target, alphas)

    def composed():
        g = F @ W.T + b
        return torch.stack([((base + a * g).argmax(1) == target).sum() for a in alphas])

    res = {"B": SEARCH_ROWS, "C": C, "d": d, "cells": alphas.numel(), "hits_equal": bool((fused() == composed()).all())}
    _alternate(res, "search", fused, composed, calls)
    g = ops.gemm_nt(F, W, bias=b, split_k=False)
    res["search_launch_alone"] = _q([_time(lambda: ops.gda_search(g, base, target, alphas)) for _ in range(calls)])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gda", "bench_gda.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    ok, why = device_linalg_works(dev)
    out = {"device": torch.cuda.get_device_name(0), "calls": args.calls, "torch_device_linalg": ok}
    if not ok:
        out["torch_device_linalg_error"] = why
    for i, (C, d, per) in enumerate(SHAPES):
        res, state = run(C, d, per, args.calls, dev, ok)
        out[f"C{C}_d{d}_s{per}"] = res
        if i == 0:
            out["search"] = run_search(C, d, state, args.calls, dev)
        print(json.dumps({f"C{C}_d{d}_s{per}": res}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
    print(json.dumps({"search": out["search"]}), flush=True)


if __name__ == "__main__":
    main()
