"""Times the symmetric CLIP pair objective with a device-side scale (csrc/clip_pairs.hip) against the route the tree had
before it and against the sigmoid loss it stands beside.

(a) the symmetric loss and the gradients of R queries x N keys at s = 100:
        clip      ONE call of ops.clip_pairs_objective (weight_k != 0) with all three gradients (dq, dk, d log s)
        infonce   two calls of ops.contrastive_objective: the same loss with both feature gradients, s a host constant
        sigmoid   one call of ops.sigmoid_objective at (t, b) = (10, -10) with its three gradients
    at the shapes of scripts/bench_contrastive.py, with the number of kernels each arm launches (torch profiler), the rows
    grid of the clip arm and the largest difference between the clip and the infonce results.
(b) one LoRAPairTrainer.step_pairs at the cfg-2 geometry (bench_contrastive.py's) under pair_loss="clip" with a trained
    head against pair_loss="infonce".

The arms alternate call by call in one process, warm; each call is timed with a pair of events on the stream and the
medians over ``--calls`` calls are reported with minimum and maximum, whatever they are: no ratio is promised.

    python scripts/bench_clip_pairs.py [--calls 20] [--skip-step] [--out profiles/clip_pairs/bench_clip_pairs.json]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "jittor-clip-fewshot_amd"), ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from bench_contrastive import S, SHAPES, _inputs, alternate, count_kernels  # noqa: E402
from bench_contrastive import fused as infonce  # noqa: E402
from bench_sigmoid import _trainer  # noqa: E402
from bench_sigmoid import sigmoid  # noqa: E402


def clip(q, k, qg, kg, head):
    from clipfs import ops
    loss, _, _, _, dq, dk, dhead = ops.clip_pairs_objective(q, k, qg, kg, head, 0.5 / q.shape[0], 0.5 / k.shape[0])
    return loss, dq, dk, dhead


def bench_objective(R, N, d, calls, dev):
    from clipfs import ops
    q, k, qg, kg = _inputs(R, N, d, 1, dev)
    head = torch.tensor([math.log(S)], device=dev)
    shead = torch.tensor([math.log(10.0), -10.0], device=dev)
    a, b = clip(q, k, qg, kg, head), infonce(q, k, qg, kg)
    diff = {"loss": abs(a[0].item() - b[0].item()),
            "dq_share": ((a[1] - b[1]).abs().max() / b[1].abs().max()).item(),
            "dk_share": ((a[2] - b[2]).abs().max() / b[2].abs().max()).item()}
    arms = {"clip": lambda: clip(q, k, qg, kg, head), "infonce": lambda: infonce(q, k, qg, kg),
            "sigmoid": lambda: sigmoid(q, k, qg, kg, shead)}
    t = alternate(arms, calls)
    out = {"R": R, "N": N, "d": d, **t,
           "infonce_over_clip": round(t["infonce"]["ms"] / t["clip"]["ms"], 3),
           "sigmoid_over_clip": round(t["sigmoid"]["ms"] / t["clip"]["ms"], 3),
           "kernels": {name: count_kernels(fn) for name, fn in arms.items()},
           "rows_kernel_workgroups": ops.clip_pairs_plan("rows", R, N, d, True)["grid"][0],
           "feat_chunk": {op: ops.clip_pairs_plan(op, R, N, d, True)["feat_chunk"] for op in ("dq", "dk")},
           "clip_minus_infonce": diff}
    print(f"[bench_clip_pairs] objective {R} x {N} x {d}: clip {t['clip']['ms']} ms, infonce {t['infonce']['ms']} ms, "
          f"sigmoid {t['sigmoid']['ms']} ms, kernels {out['kernels']}", file=sys.stderr)
    return out


def bench_step(calls, dev):
    from clipfs import synth
    tr_c, cfg = _trainer(dev, pair_loss="clip", train_pair_head=True)
    tr_i, _ = _trainer(dev)
    Bn = M = 256
    img = synth.synth_images(Bn, 224, seed=0).to(dev)
    cap = synth.synth_captions(M, 77, cfg.vocab_size, seed=1).to(dev)
    arms = {"clip": lambda: tr_c.step_pairs(img, cap), "infonce": lambda: tr_i.step_pairs(img, cap)}
    t = alternate(arms, calls)
    out = {"geometry": "cfg-2: ViT-B/32, rank-4 LoRA q,k,v on 12 + 12 blocks, 4 prompt tokens, dropout 0.25, 256 images, "
                       "256 captions (pairs); clip: trained head, decay 0, clamp at log 100", "step_pairs": t,
           "ratio_clip_over_infonce": round(t["clip"]["ms"] / t["infonce"]["ms"], 4),
           "kernels": {name: count_kernels(fn) for name, fn in arms.items()},
           "scale_after": tr_c.pair_scale_value}
    print(f"[bench_clip_pairs] step_pairs clip {t['clip']['ms']} ms, infonce {t['infonce']['ms']} ms", file=sys.stderr)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--skip-step", action="store_true", help="the objective alone, without the cfg-2 training step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_pairs", "bench_clip_pairs.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_clip_pairs.py needs an MI355X"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "calls": args.calls, "logit_scale": S,
           "objective": [bench_objective(R, N, d, args.calls, dev) for R, N, d in SHAPES]}
    if not args.skip_step:
        res["step"] = bench_step(max(args.calls // 2, 5), dev)
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
