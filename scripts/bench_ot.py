"""Times the OT matching (csrc/ot_match.hip; ``ops.ot_logits``, ``ops.ot_bwd``) against the same rule composed in torch
on the device: ``einsum`` for z, ``exp``, the loop of element-wise products and sums of the Sinkhorn iterations, ``einsum``
for the two gradients.

Shapes (B, M, C, N, d): (256, 49, 403, 4, 512) and (256, 196, 1000, 4, 512), 100 iterations, eps 0.1.  Both routes
alternate in one process, warm; every timing is a pair of events on the stream, medians over ``--calls`` calls with min
and max.  Launch counts: the plan's on this side; on the torch side the operations of the composition as written (each at
least one launch).  ``python bench.py`` runs nothing of this.

    python scripts/bench_ot.py [--calls 7] [--out profiles/ot/bench_ot.json]
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

SHAPES = ((256, 49, 403, 4, 512), (256, 196, 1000, 4, 512))
EPS, ITERS, SCALE = 0.1, 100, 100.0


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _q(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_max_ms": [round(min(xs), 4), round(max(xs), 4)], "calls": len(xs)}


def _unit(x):
    return x / x.norm(dim=-1, keepdim=True)


def torch_forward(X, P, eps, iters, scale):
    """(logits, T): the rule composed in torch.  1 einsum + 2 for K + per iteration 2 products, 2 sums and 2 divisions + 3 for
    T and the score: 6 iters + 6 operations."""
    B, M, _ = X.shape
    C, N, _ = P.shape
    z = torch.einsum("bmd,cnd->bcmn", X, P)
    K = torch.exp((z - 1.0) / eps)
    mu = torch.full((B, 1, M), 1.0 / M, device=X.device)
    nu = torch.full((1, C, N), 1.0 / N, device=X.device)
    v = torch.ones(B, C, N, device=X.device)
    u = None
    for _ in range(iters):
        u = mu / (K * v[:, :, None, :]).sum(3)
        v = nu / (K * u[:, :, :, None]).sum(2)
    T = u[:, :, :, None] * K * v[:, :, None, :]
    return scale * (T * z).sum((2, 3)), T


def torch_backward(X, P, T, dlogits, scale):
    G = (dlogits * scale)[:, :, None, None] * T
    return torch.einsum("bcmn,bmd->cnd", G, X), torch.einsum("bcmn,cnd->bmd", G, P)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ot", "bench_ot.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ot.py needs an MI355X")
    from clipfs import ops
    dev = torch.device("cuda:0")
    results = {"device": torch.cuda.get_device_name(0), "eps": EPS, "iters": ITERS, "scale": SCALE, "shapes": []}
    for B, M, C, N, d in SHAPES:
        g = torch.Generator().manual_seed(B + M + C)
        common = _unit(torch.randn(d, generator=g)) * d ** 0.5
        X = _unit(torch.randn(B, M, d, generator=g) + 3 * common).to(dev)
        P = _unit(torch.randn(C, N, d, generator=g) + 3 * common).to(dev)
        dl = torch.randn(B, C, generator=g).to(dev)
        plan = ops.ot_plan(B, M, C, N, d)
        state = {}

        def ours_fwd():
            state["f"] = ops.ot_logits(X, P, None, None, EPS, ITERS, SCALE)

        def ours_dp():
            _, u, v = state["f"]
            state["dp"] = ops.ot_bwd(X, P, u, v, dl, EPS, SCALE)[0]

        def ours_dx():  # the call launches dP too: dX alone is this minus dP
            _, u, v = state["f"]
            state["dx"] = ops.ot_bwd(X, P, u, v, dl, EPS, SCALE, want_dx=True)[1]

        def ref_fwd():
            state["r"] = torch_forward(X, P, EPS, ITERS, SCALE)

        def ref_bwd():
            state["rb"] = torch_backward(X, P, state["r"][1], dl, SCALE)

        for fn in (ours_fwd, ours_dp, ours_dx, ref_fwd, ref_bwd):  # warm
            fn()
        torch.cuda.synchronize()
        t = {k: [] for k in ("fwd", "dp", "dp_dx", "torch_fwd", "torch_bwd")}
        for _ in range(args.calls):  # the two routes alternate
            t["fwd"].append(_time(ours_fwd))
            t["torch_fwd"].append(_time(ref_fwd))
            t["dp"].append(_time(ours_dp))
            t["dp_dx"].append(_time(ours_dx))
            t["torch_bwd"].append(_time(ref_bwd))
        lg, rl = state["f"][0], state["r"][0]
        rdp, rdx = state["rb"]
        entry = {
            "shape": {"B": B, "M": M, "C": C, "N": N, "d": d},
            "plan": plan,
            "launches": {"fwd": plan["fwd_launches"], "dp": plan["dp_launches"], "dx": plan["dx_launches"],
                         "torch_fwd_ops": 6 * ITERS + 6, "torch_bwd_ops": 4},
            "torch_z_bytes": 4 * B * C * M * N,
            "agreement": {"logits": float((lg - rl).abs().max() / rl.abs().max()),
                          "dP": float((state["dp"] - rdp).abs().max() / rdp.abs().max()),
                          "dX": float((state["dx"] - rdx).abs().max() / rdx.abs().max())},
            "timing": {k: _q(v) for k, v in t.items()},
        }
        results["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
        del state
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
