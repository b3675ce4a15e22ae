"""Times the kernel ridge head (csrc/krr.hip on csrc/spd.hip; ``ops.krr_fit``, ``ops.krr_apply``,
``ops.spd_factor_panels``, ``ops.spd_solve_panels``) against the same rule composed in torch on the device:
``torch.exp(-beta * (1 - S @ S.T))``, ``torch.linalg.cholesky``, ``torch.cholesky_solve``, ``torch.exp(...) @ alpha``.

Shapes: the fit at d 512 for (n 1024, C 64), (n 6352, C 397) and (n 16 000, C 1000); the apply at B 8192 on each; factor
and solve alone at panel 128 / 256 / 512 (the fused pair at n 1024) against torch's.  Both routes alternate in one
process, warm; every timing is a pair of events on the stream, medians over ``--calls`` calls with min and max, beside the
plan's launch counts and the stages of a fit alone.  ``python bench.py`` runs nothing of this.

    python scripts/bench_proker.py [--calls 7] [--shapes 1024x64,6352x397,16000x1000] [--out profiles/proker/bench_proker.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "jittor-clip-fewshot_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

D, ROWS, BETA, LAM = 512, 8192, 5.5, 1.0
PANELS = (128, 256, 512)


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _q(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_max_ms": [round(min(xs), 4), round(max(xs), 4)], "calls": len(xs)}


def _alternate(res, name, ours, composed, calls):
    ours()
    composed()
    to, tc = [], []
    for _ in range(calls):
        to.append(_time(ours))
        tc.append(_time(composed))
    res[name] = {"ours": _q(to), "composed": _q(tc), "composed_over_ours": round(statistics.median(tc) / statistics.median(to), 3)}


def make(n, C, dev, seed=0):
    gen = torch.Generator(dev).manual_seed(seed)
    unit = lambda x: torch.nn.functional.normalize(x, dim=-1)
    rn = lambda *s: torch.randn(*s, device=dev, generator=gen)
    centres = unit(rn(C, D))
    labels = (torch.arange(n, device=dev) % C).to(torch.int32)
    S = unit(centres[labels.long()] + 0.5 * rn(n, D) / D ** 0.5).contiguous()
    target = torch.randint(0, C, (ROWS,), device=dev, generator=gen)
    X = unit(centres[target] + 0.5 * rn(ROWS, D) / D ** 0.5).contiguous()
    T = unit(centres + 0.5 * rn(C, D) / D ** 0.5)
    return S, labels, X, (S @ T.T).contiguous(), (X @ T.T).contiguous()


class Composed:
    """The rule on torch."""

    def __init__(self, S, labels, C, base_S):
        self.S, self.C = S, C
        self.Y = torch.nn.functional.one_hot(labels.long(), C).float() - base_S

    def system(self):
        S = self.S
        self.A = torch.exp(-BETA * (1 - S @ S.T)) + LAM * torch.eye(S.shape[0], device=S.device)

    def factor(self):
        self.L = torch.linalg.cholesky(self.A)

    def solve(self):
        self.alpha = torch.cholesky_solve(self.Y, self.L)

    def fit(self):
        self.system()
        self.factor()
        self.solve()

    def apply(self, X, base):
        return base + torch.exp(-BETA * (1 - X @ self.S.T)) @ self.alpha


def run(n, C, calls, dev):
    from clipfs import ops
    S, labels, X, base_S, base = make(n, C, dev)
    host = labels.cpu()
    plan = ops.krr_plan(n, C, D, ROWS, 256)
    res = {"n": n, "C": C, "d": D, "B": ROWS, "beta": BETA, "lambda": LAM, "panelled": plan["panelled"],
           "fit_launches_plan": plan["fit_launches"], "factor_launches_plan": plan["factor_launches"],
           "solve_launches_plan": plan["solve_launches"], "apply_tiles_per_wave": plan["tiles_per_wave"],
           "apply_grid": [plan["apply_grid_x"], plan["apply_grid_y"]]}
    comp = Composed(S, labels, C, base_S)
    bufs = ops.krr_buffers(n, C, dev)
    ours_fit = lambda: ops.krr_fit(S, labels, C, base_S, BETA, LAM, 1.0, 256, labels_host=host, buffers=bufs)
    ours_fit()
    comp.fit()
    torch.cuda.synchronize()
    res["info"] = int(bufs["info"].item())
    At = bufs["At"][:, :n]
    res["max_rel_diff_At_ours_vs_composed"] = float((At - comp.alpha.T).abs().max() / comp.alpha.abs().max())
    _alternate(res, "fit", ours_fit, comp.fit, calls)
    out = torch.empty(ROWS, C, device=dev)
    ours_apply = lambda: ops.krr_apply(X, S, bufs["At"], base, BETA, out=out)
    ours_apply()
    ref = comp.apply(X, base)
    res["max_abs_diff_logits_ours_vs_composed"] = float((out - ref).abs().max())
    del ref
    _alternate(res, "apply", ours_apply, lambda: comp.apply(X, base), calls)
    # where the time goes: the stages alone, on the fit's own buffers
    A = bufs["A"].clone()
    for name, fn in {"system": lambda: ops.krr_system(S, BETA, LAM, out=A),
                     "targets": lambda: ops.krr_targets(labels, C, base_S, 1.0, out=bufs["Et"])}.items():
        fn()
        res["stage_" + name] = _q([_time(fn) for _ in range(calls)])
    comp.system()
    res["stage_system_composed"] = _q([_time(comp.system) for _ in range(calls)])
    chol, Xo = torch.empty_like(A), torch.empty_like(bufs["At"])
    if plan["panelled"]:
        for panel in PANELS:
            sp = ops.spd_panels_plan(plan["n4"], C, panel)
            _alternate(res, f"factor_panel{panel}", lambda: ops.spd_factor_panels(A, out=chol, panel=panel), comp.factor, calls)
            _alternate(res, f"solve_panel{panel}", lambda: ops.spd_solve_panels(chol, bufs["Et"], out=Xo, panel=panel), comp.solve,
                       calls)
            res[f"plan_panel{panel}"] = {k: sp[k] for k in ("panels", "band", "factor_launches", "factor_gemms", "solve_launches",
                                                            "solve_gemms")}
    else:
        _alternate(res, "factor_fused", lambda: ops.spd_factor(A, out=chol), comp.factor, calls)
        _alternate(res, "solve_fused", lambda: ops.spd_solve(chol, bufs["Et"], out=Xo), comp.solve, calls)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--shapes", default="1024x64,6352x397,16000x1000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "proker", "bench_proker.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "calls": args.calls}
    for shape in args.shapes.split(","):
        n, C = (int(v) for v in shape.split("x"))
        out[f"n{n}_C{C}"] = run(n, C, args.calls, dev)
        print(json.dumps({f"n{n}_C{C}": out[f"n{n}_C{C}"]}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
