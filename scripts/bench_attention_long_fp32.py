"""Exact-fp32 attention past 288 tokens: the long-sequence MFMA kernels (the default path of ops.attention_fwd / _bwd up to
ops.attention_mfma_max_seq() tokens) against the streaming VALU kernels, which ran these lengths before.

    python scripts/bench_attention_long_fp32.py [--shape B,H,L ...] [--rounds 7] [--iters 3] [--json OUT]

Default shapes: 64 x 16 heads x 577 tokens (ViT-L/14 at 336 px, 64 images) and 16 x 16 heads x 1024 tokens, forward (with
lse) and backward.  CLIPFS_ATTN_MFMA is read once per process, so each leg runs in a fresh child process under its own
`timeout`: first the default path, then the same calls with CLIPFS_ATTN_MFMA=0.  This process never opens the GPU.  A leg
that fails ends the run: nothing more is started.  HIP events around `iters` calls, two warm-up calls per arm, median and
minimum over `rounds`.  Prints one JSON line (and writes it to --json)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jittor-clip-fewshot_amd"))
sys.path.insert(0, ROOT)

DEFAULT_SHAPES = ["64,16,577", "16,16,1024"]
LEG_TIMEOUT_S = 240


def _timed(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us


def leg(args):
    """One process = one setting of CLIPFS_ATTN_MFMA: times forward and backward at every shape."""
    import torch
    from clipfs import ops
    dev = torch.device("cuda:0")
    res = {"CLIPFS_ATTN_MFMA": os.environ.get("CLIPFS_ATTN_MFMA", ""), "device": torch.cuda.get_device_name(0), "shapes": {}}
    for shape in args.shape:
        B, H, L = (int(v) for v in shape.split(","))
        g = torch.Generator().manual_seed(1)
        qkv = torch.randn(B * L, 3 * H * 64, generator=g).to(dev)  # random data: zeros would flatter the softmax
        dout = torch.randn(B * L, H * 64, generator=g).to(dev)
        out, lse = ops.attention_fwd(qkv, B, L, H, False, want_lse=True)
        arms = {"fwd": lambda: ops.attention_fwd(qkv, B, L, H, False, want_lse=True),
                "bwd": lambda: ops.attention_bwd(qkv, dout, B, L, H, False, out=out, lse=lse)}
        for fn in arms.values():  # warm-up: first-launch costs and clocks
            fn()
            fn()
        torch.cuda.synchronize()
        us = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, fn in arms.items():
                us[k].append(_timed(fn, args.iters))
        fl = 4 * L * L * 64 * B * H  # forward; the backward is priced at 2.5 x
        res["shapes"][shape] = {
            k: {"median": round(statistics.median(v), 1), "min": round(min(v), 1),
                "tflops_at_median": round(fl * (2.5 if k == "bwd" else 1.0) / statistics.median(v) / 1e6, 1)}
            for k, v in us.items()}
        # a checksum of what was timed, so that the two legs can be seen to compute the same function
        dqkv = ops.attention_bwd(qkv, dout, B, L, H, False, out=out, lse=lse)
        res["shapes"][shape]["out_abs_sum"] = out.double().abs().sum().item()
        res["shapes"][shape]["dqkv_abs_sum"] = dqkv.double().abs().sum().item()
    print(json.dumps(res), flush=True)


def _run_leg(args, mfma):
    env = dict(os.environ)
    env["CLIPFS_ATTN_MFMA"] = "1" if mfma else "0"
    cmd = ["timeout", "-k", "10", str(LEG_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--leg", "--rounds",
           str(args.rounds), "--iters", str(args.iters)]
    for s in args.shape:
        cmd += ["--shape", s]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        sys.exit(f"leg CLIPFS_ATTN_MFMA={env['CLIPFS_ATTN_MFMA']} ended with status {r.returncode}: nothing more is started")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", metavar="B,H,L", help="batch,heads,tokens (repeatable)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--leg", action="store_true", help="(internal) time this process's setting of CLIPFS_ATTN_MFMA")
    ap.add_argument("--json", metavar="OUT")
    args = ap.parse_args()
    args.shape = args.shape or DEFAULT_SHAPES
    if args.leg:
        return leg(args)
    mfma = _run_leg(args, True)
    valu = _run_leg(args, False)
    res = {"mode": "kernels_fp32", "unit": "us", "rounds": args.rounds, "iters_per_round": args.iters, "device": mfma["device"],
           "shapes": {}}
    for s in args.shape:
        a, b = mfma["shapes"][s], valu["shapes"][s]
        res["shapes"][s] = {
            "fwd_mfma_long": a["fwd"], "fwd_streaming": b["fwd"], "bwd_mfma_long": a["bwd"], "bwd_streaming": b["bwd"],
            "fwd_speedup_median": round(b["fwd"]["median"] / a["fwd"]["median"], 2),
            "bwd_speedup_median": round(b["bwd"]["median"] / a["bwd"]["median"], 2),
            "out_abs_sum": [a["out_abs_sum"], b["out_abs_sum"]], "dqkv_abs_sum": [a["dqkv_abs_sum"], b["dqkv_abs_sum"]]}
    line = json.dumps(res)
    print(line, flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
