"""Times the Tip-Adapter cache head (csrc/cache_head.hip) against the composed baseline built from what the tree had
before it: ``ops.gemm_nt`` for the [B, NK] affinity, torch ``exp`` / ``index_add_`` / ``argmax`` around it, and the per-cell
loop for the search.  Forward, backward, search and one trainer step, at two geometries:

    fewshot   B = 256,  C = 403,  4 shots (NK = 1612),   d = 512,  search grid 200 betas x 20 alphas
    imagenet  B = 8192, C = 1000, 16 shots (NK = 16000), d = 1024, search grid 200 betas x 20 alphas

Fused and composed alternate call by call in one process, warm; each call is timed with a pair of events on the stream
and the medians over ``--calls`` calls (at least 20) are reported, with the ratio composed / fused.

    python scripts/bench_cache_head.py [--calls 20] [--geometry fewshot imagenet] [--out FILE.json]
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

GEOMETRIES = {"fewshot": dict(B=256, C=403, shots=4, d=512, nA=20, nB=200),
              "imagenet": dict(B=8192, C=1000, shots=16, d=1024, nA=20, nB=200)}


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(fused, composed, calls, composed_calls=None):
    """Medians (ms) of ``fused`` and ``composed`` called alternately; ``composed_calls`` caps the slow side (its calls
    are spread evenly among the fused ones), never below 20."""
    composed_calls = max(20, min(calls, composed_calls or calls))
    for fn in (fused, composed, fused):
        fn()
    torch.cuda.synchronize()
    tf, tc = [], []
    every = max(1, calls // composed_calls)
    for k in range(calls):
        tf.append(_time(fused))
        if k % every == 0 and len(tc) < composed_calls:
            tc.append(_time(composed))
    while len(tc) < composed_calls:
        tf.append(_time(fused))
        tc.append(_time(composed))
    q = lambda xs: (min(xs), statistics.median(xs), max(xs))
    f, c = q(tf), q(tc)
    return {"fused_ms": round(f[1], 4), "fused_min_max_ms": [round(f[0], 4), round(f[2], 4)], "fused_calls": len(tf),
            "composed_ms": round(c[1], 4), "composed_min_max_ms": [round(c[0], 4), round(c[2], 4)], "composed_calls": len(tc),
            "composed_over_fused": round(c[1] / f[1], 2)}


def run(name, g, calls, dev):
    from clipfs import ops
    from tip_adapter import TipAdapter, TipAdapterTrainer
    B, C, shots, d, nA, nB = (g[k] for k in ("B", "C", "shots", "d", "nA", "nB"))
    NK = C * shots
    gen = torch.Generator(dev).manual_seed(0)
    unit = lambda *s: torch.nn.functional.normalize(torch.randn(*s, device=dev, generator=gen), dim=1)
    proto = unit(C, d)
    labels = torch.arange(C, device=dev).repeat_interleave(shots)
    K = torch.nn.functional.normalize(proto[labels] + 0.05 * torch.randn(NK, d, device=dev, generator=gen), dim=1)
    y = torch.randint(0, C, (B,), device=dev, generator=gen)
    f = torch.nn.functional.normalize(proto[y] + 0.08 * torch.randn(B, d, device=dev, generator=gen), dim=1)
    text = torch.nn.functional.normalize(proto + 0.05 * torch.randn(C, d, device=dev, generator=gen), dim=1)
    base = ops.gemm_nt(f, text) * 100.0
    off = torch.arange(0, NK + 1, shots, device=dev, dtype=torch.int32)
    dl = torch.randn(B, C, device=dev, generator=gen) / B
    alpha, beta = 1.0, 5.5
    alphas = torch.linspace(0.0, 3.0, nA, device=dev)
    betas = torch.linspace(0.5, 7.0, nB, device=dev)
    alist, blist = alphas.tolist(), betas.tolist()
    fT = f.t().contiguous()

    def composed_S(bt):
        E = torch.exp(-bt * (1.0 - ops.gemm_nt(f, K)))
        return E, torch.zeros(B, C, device=dev).index_add_(1, labels, E)

    def composed_fwd():
        return base + alpha * composed_S(beta)[1]

    dK_f, dK_c = torch.zeros_like(K), torch.zeros_like(K)

    def fused_bwd():
        return ops.cache_bwd(f, K, off, dl, dK_f, alpha, beta, want_df=True)

    def composed_bwd():
        E, _ = composed_S(beta)
        G = (alpha * beta) * E * dl.index_select(1, labels)
        dK_c.add_(ops.gemm_nt(G.t().contiguous(), fT))
        return ops.gemm_nt(G, K.t().contiguous())

    def composed_search():
        hits = torch.zeros(nB, nA, device=dev, dtype=torch.int32)
        for j, bt in enumerate(blist):
            S = composed_S(bt)[1]
            for i, al in enumerate(alist):
                hits[j, i] = ((base + al * S).argmax(1) == y).sum()
        return hits

    tr = TipAdapterTrainer(TipAdapter.from_features(K, labels, C, alpha, beta))
    pc, gc = K.clone().view(-1), torch.zeros(NK * d, device=dev)
    mc, vc = torch.zeros_like(gc), torch.zeros_like(gc)
    step = [0]

    def composed_step():
        Kc = pc.view(NK, d)
        E = torch.exp(-beta * (1.0 - ops.gemm_nt(f, Kc)))
        logits = base + alpha * torch.zeros(B, C, device=dev).index_add_(1, labels, E)
        loss, dlog, correct = ops.cross_entropy(logits, y)
        G = (alpha * beta) * E * dlog.index_select(1, labels)
        ops.gemm_nt(G.t().contiguous(), fT, out=gc.view(NK, d))
        step[0] += 1
        ops.adamw_ext(pc, gc, mc, vc, step[0], 1e-3, (0.9, 0.999), 1e-4, 1e-2)
        return loss, correct

    res = {"geometry": dict(g, NK=NK)}
    # the two sides compute the same thing (the composed search is the slow oracle of the fused one)
    err = float((ops.cache_logits(f, K, off, base, alpha, beta) - composed_fwd()).abs().max())
    res["fwd_max_abs_diff_vs_composed"] = err
    res["forward"] = alternate(lambda: ops.cache_logits(f, K, off, base, alpha, beta), composed_fwd, calls)
    res["backward_dK_df"] = alternate(fused_bwd, composed_bwd, calls)
    res["trainer_step"] = alternate(lambda: tr.step(f, base, y), composed_step, calls)
    h_f = ops.cache_search(f, K, off, base, y, alphas, betas)
    h_c = composed_search()
    res["search_cells_differing_vs_composed"] = int((h_f != h_c).sum())
    res["search"] = alternate(lambda: ops.cache_search(f, K, off, base, y, alphas, betas), composed_search, calls, 20)
    res["search_plan"] = {k: v for k, v in ops.cache_plan("search", B, NK, C, d, nA, nB).items()}
    print(json.dumps({name: res}), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--geometry", nargs="+", default=list(GEOMETRIES), choices=list(GEOMETRIES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "calls": max(20, args.calls)}
    for name in args.geometry:
        out[name] = run(name, GEOMETRIES[name], max(20, args.calls), dev)
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
