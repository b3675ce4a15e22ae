"""Times the sigmoid (SigLIP) objective (csrc/sigmoid_pairs.hip) against the route composed from what the tree had before
it and against the symmetric InfoNCE loss it stands beside.

(a) the loss, the gradients of both feature sides and of the head (log t, b) of R queries x N keys, (t, b) = (10, -10):
        sigmoid   one call of ops.sigmoid_objective
        composed  ops.gemm_nt for the [R, N] logits, torch for the masks, logsigmoid, the logits gradient and the two head
                  sums, two ops.matmul_small for the feature gradients
        infonce   two calls of ops.contrastive_objective: the symmetric InfoNCE loss with both gradients (no head)
    at the shapes of scripts/bench_contrastive.py, with the number of kernels each arm launches and the largest difference
    between the sigmoid and the composed results.
(b) one LoRAPairTrainer.step_pairs at the cfg-2 geometry (bench_contrastive.py's) under pair_loss="sigmoid" with a
    trained head against pair_loss="infonce".

The arms alternate call by call in one process, warm; each call is timed with a pair of events on the stream and the
medians over ``--calls`` calls are reported with minimum and maximum, whatever they are.

    python scripts/bench_sigmoid.py [--calls 20] [--skip-step] [--out profiles/sigmoid/bench_sigmoid.json]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "jittor-clip-fewshot_amd"), ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from bench_contrastive import SHAPES, _inputs, alternate, count_kernels  # noqa: E402
from bench_contrastive import fused as infonce  # noqa: E402

T, B = 10.0, -10.0


def sigmoid(q, k, qg, kg, head):
    from clipfs import ops
    loss, _, _, dq, dk, dhead = ops.sigmoid_objective(q, k, qg, kg, head, 1.0 / q.shape[0])
    return loss, dq, dk, dhead


def composed(q, k, qg, kg):
    from clipfs import ops
    R, d = q.shape
    N = k.shape[0]
    w = 1.0 / R
    z = ops.gemm_nt(q, k, alpha=T) + B
    live = (qg[:, None] >= 0) & (kg[None, :] >= 0)
    pos = live & (qg[:, None] == kg[None, :])
    cell = -torch.nn.functional.logsigmoid(torch.where(pos, z, -z))
    loss = w * torch.where(live, cell, torch.zeros_like(cell)).sum()
    G = torch.where(live, w * (torch.sigmoid(z) - pos.float()), torch.zeros_like(z)).contiguous()
    dq = ops.matmul_small(G, k, R, d, N, N, 1, d, 1, T)
    dk = ops.matmul_small(G, q, N, d, R, 1, N, d, 1, T)
    dhead = torch.stack([(G * (z - B)).sum(), G.sum()])  # t G a = G (z - b)
    return loss, dq, dk, dhead


def bench_objective(R, N, d, calls, dev):
    q, k, qg, kg = _inputs(R, N, d, 1, dev)
    head = torch.tensor([math.log(T), B], device=dev)
    a, b = sigmoid(q, k, qg, kg, head), composed(q, k, qg, kg)
    diff = {"loss_rel": abs(a[0].item() - b[0].item()) / abs(b[0].item()),
            "dq_share": ((a[1] - b[1]).abs().max() / b[1].abs().max()).item(),
            "dk_share": ((a[2] - b[2]).abs().max() / b[2].abs().max()).item(),
            "dhead_rel": ((a[3] - b[3]).abs() / b[3].abs()).max().item()}
    arms = {"sigmoid": lambda: sigmoid(q, k, qg, kg, head), "composed": lambda: composed(q, k, qg, kg),
            "infonce": lambda: infonce(q, k, qg, kg)}
    t = alternate(arms, calls)
    out = {"R": R, "N": N, "d": d, **t,
           "composed_over_sigmoid": round(t["composed"]["ms"] / t["sigmoid"]["ms"], 3),
           "infonce_over_sigmoid": round(t["infonce"]["ms"] / t["sigmoid"]["ms"], 3),
           "kernels": {name: count_kernels(fn) for name, fn in arms.items()},
           "rows_kernel_workgroups": -(-R // 32), "sigmoid_minus_composed": diff}
    print(f"[bench_sigmoid] objective {R} x {N} x {d}: sigmoid {t['sigmoid']['ms']} ms, composed {t['composed']['ms']} ms, "
          f"infonce {t['infonce']['ms']} ms, kernels {out['kernels']}", file=sys.stderr)
    return out


def _trainer(dev, **kw):
    import contextlib

    import lora_train_vlp as L
    from clipfs import synth
    from jclip.model import build_model
    cfg = synth.VIT_B32
    model = build_model(synth.synth_state_dict(cfg, seed=1234), device=dev)
    largs = types.SimpleNamespace(encoder="both", position="all", backbone="ViT-B/32", params=["q", "k", "v"], r=4, alpha=1,
                                  dropout_rate=0.25)
    layers = L.apply_lora(largs, model)
    with contextlib.redirect_stdout(sys.stderr):
        L.load_lora(largs, layers, os.path.join(ROOT, "tests", "golden", "lora_weights.pkl"))
    L.mark_only_lora_as_trainable(model)
    ids = torch.tensor([320, 1125, 539, 320], device=dev)
    ctx = torch.nn.Parameter(model.token_embedding.weight.data[ids].clone())
    model.train()
    return L.LoRAPairTrainer(model, prompt_ctx=ctx, **kw), cfg


def bench_step(calls, dev):
    from clipfs import synth
    tr_s, cfg = _trainer(dev, pair_loss="sigmoid", train_pair_head=True)
    tr_i, _ = _trainer(dev)
    Bn = M = 256
    img = synth.synth_images(Bn, 224, seed=0).to(dev)
    cap = synth.synth_captions(M, 77, cfg.vocab_size, seed=1).to(dev)
    arms = {"sigmoid": lambda: tr_s.step_pairs(img, cap), "infonce": lambda: tr_i.step_pairs(img, cap)}
    t = alternate(arms, calls)
    out = {"geometry": "cfg-2: ViT-B/32, rank-4 LoRA q,k,v on 12 + 12 blocks, 4 prompt tokens, dropout 0.25, 256 images, "
                       "256 captions (pairs); sigmoid: trained head", "step_pairs": t,
           "ratio_sigmoid_over_infonce": round(t["sigmoid"]["ms"] / t["infonce"]["ms"], 4),
           "kernels": {name: count_kernels(fn) for name, fn in arms.items()}}
    print(f"[bench_sigmoid] step_pairs sigmoid {t['sigmoid']['ms']} ms, infonce {t['infonce']['ms']} ms", file=sys.stderr)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--skip-step", action="store_true", help="the objective alone, without the cfg-2 training step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sigmoid", "bench_sigmoid.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sigmoid.py needs an MI355X"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "calls": args.calls, "head": {"t": T, "b": B},
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
