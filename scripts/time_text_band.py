"""Stand-alone timing of the packed text tower's GEMM band: the eight products [R, N, K] a text block runs on R live rows
(forward and backward, with the epilogue each one carries in the tower) and the image tower's shapes at M = 12 800.
Every product is timed warm in two settings:

  alone  -- `reps` back-to-back launches on one stream;
  beside -- the same launches while a [12 800, 768, 3072] product loops on a second stream for the whole window.  Reported
            is the MARGINAL time: (both streams' makespan - the image loop alone) / launches, i.e. what the product adds
            to a step whose other tower keeps the matrix cores busy.

One JSON document on stdout (and in --out): per product us alone, fraction of the 157.3 TFLOP/s fp32 MFMA peak, marginal us
beside the image loop, the host queries' answers, and the per-step totals weighted by launches per step (11 text blocks).

    python scripts/time_text_band.py [--rows 9748] [--reps 40] [--out FILE]

Library variants are compared by running it once per variant (CLIPFS_LIB_TAG / the tuning aids are read once per process).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jittor-clip-fewshot_amd"))

PEAK = 157.3e12
# name, N, K, launches per text block, epilogue
TEXT_PRODUCTS = [
    ("out_fwd", 512, 512, 1, "bias_res"),
    ("c_proj_fwd", 512, 2048, 1, "bias_res"),
    ("c_fc_dgrad", 512, 2048, 1, "plain"),
    ("out_dgrad", 512, 512, 1, "plain"),
    ("qkv_dgrad", 512, 1536, 1, "res"),
    ("c_fc_fwd", 2048, 512, 1, "bias_gelu_aux"),
    ("c_proj_dgrad", 2048, 512, 1, "gelu_grad"),
    ("qkv_fwd", 1536, 512, 1, "bias"),
]
IMAGE_PRODUCTS = [("img_n768_k768", 768, 768), ("img_n2304_k768", 2304, 768), ("img_n3072_k768", 3072, 768),
                  ("img_n768_k3072", 768, 3072)]
TEXT_BLOCKS = 11


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=9748)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--image-loop", type=int, default=16)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    from clipfs import _lib, ops
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    s0 = torch.cuda.current_stream()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()

    def make(M, N, K, epi):
        a = torch.randn(M, K, device=dev)
        b = torch.randn(N, K, device=dev)
        c = torch.empty(M, N, device=dev)
        kw = {}
        if "bias" in epi:
            kw["bias"] = torch.randn(N, device=dev)
        if "res" in epi:
            kw["residual"] = torch.randn(M, N, device=dev)
        if epi == "bias_gelu_aux":
            kw.update(act=1, aux_out=torch.empty(M, N, device=dev))
        if epi == "gelu_grad":
            kw.update(act=2, aux_in=torch.randn(M, N, device=dev))
        return lambda: ops.gemm_nt(a, b, c, **kw)

    def window(on1, n1, on2, n2):
        """ms from a common start until both streams are done: n1 x on1 on s1 beside n2 x on2 on s2"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(s0)
        s1.wait_stream(s0)
        s2.wait_stream(s0)
        with torch.cuda.stream(s2):
            for _ in range(n2):
                on2()
        with torch.cuda.stream(s1):
            for _ in range(n1):
                on1()
        s0.wait_stream(s1)
        s0.wait_stream(s2)
        e1.record(s0)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    # the first seconds of a process run at a lower clock: warm up on the image loop's product
    img = make(12800, 768, 3072, "bias")
    for _ in range(400):
        img()
    torch.cuda.synchronize()
    L = args.image_loop
    img_ms = min(window(img, 0, img, L) for _ in range(3))

    rows = []
    jobs = [(n, args.rows, N, K, w * TEXT_BLOCKS, e) for n, N, K, w, e in TEXT_PRODUCTS] + \
           [(n, 12800, N, K, 0, "bias") for n, N, K in IMAGE_PRODUCTS]
    for name, M, N, K, per_step, epi in jobs:
        fn = make(M, N, K, epi)
        for _ in range(5):
            fn()
        alone = min(window(fn, args.reps, fn, 0) for _ in range(3)) / args.reps * 1e3  # us
        # half as much text work as the image loop lasts, so that the loop covers the whole window
        n = max(1, int(0.5 * img_ms * 1e3 / alone))
        both = min(window(fn, n, img, L) for _ in range(3))
        fl = 2.0 * M * N * K
        rows.append(dict(name=name, M=M, N=N, K=K, epilogue=epi, launches_per_step=per_step, us_alone=round(alone, 2),
                         fraction_of_peak_alone=round(fl / (alone * 1e-6) / PEAK, 4), beside_launches=n,
                         beside_makespan_ms=round(both, 4), us_marginal_beside=round((both - img_ms) / n * 1e3, 2),
                         tile_rows=lib.clipfs_gemm_tile_rows(M, N),
                         mixed_rows64=lib.clipfs_gemm_mixed_rows64(M, N, K) if hasattr(lib, "clipfs_gemm_mixed_rows64") else 0))
        print(json.dumps(rows[-1]), flush=True)
    text = [r for r in rows if r["launches_per_step"]]
    doc = dict(rows_live=args.rows, reps=args.reps, image_loop=dict(product=[12800, 768, 3072], launches=L, ms_alone=round(img_ms, 4)),
               library=os.path.basename(_lib.LIB_PATH),
               env={k: v for k, v in os.environ.items() if k.startswith("CLIPFS_")},
               text_ms_per_step_alone=round(sum(r["us_alone"] * r["launches_per_step"] for r in text) / 1e3, 3),
               text_ms_per_step_marginal_beside=round(sum(r["us_marginal_beside"] * r["launches_per_step"] for r in text) / 1e3, 3),
               products=rows)
    print(json.dumps({k: v for k, v in doc.items() if k != "products"}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
