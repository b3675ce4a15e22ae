"""The first LoRATrainer.step_pairs of a tree, dumped for a byte-for-byte comparison between two builds: loss, hit counts,
the flat gradient and the updated parameters on the suite's small test model (tests/test_contrastive_gpu.py: rank-4 q/k/v
adapters on every block, LoRA dropout 0.25, training mode), paired and grouped batches, under the default pair_loss and
under pair_loss="sigmoid" with a trained head.

    python scripts/dump_step_pairs.py --root TREE --out FILE.npz      dump the tree at TREE (default: this one)
    python scripts/dump_step_pairs.py --compare A.npz B.npz          compare two dumps; exit status 1 on any difference
    python scripts/dump_step_pairs.py --digest A.npz                 name, dtype, shape and sha256 of every array of a dump
"""
from __future__ import annotations

import argparse
import hashlib
import os
import sys

import numpy as np


class _Monkey:
    @staticmethod
    def setitem(d, k, v):
        d[k] = v


def dump(root, out):
    for p in (os.path.join(root, "jittor-clip-fewshot_amd"), root, os.path.join(root, "tests")):
        sys.path.insert(0, p)
    import torch

    import test_contrastive_gpu as TC
    dev = torch.device("cuda:0")
    arrays = {}
    for loss_name, kw in (("infonce", {}), ("sigmoid", dict(pair_loss="sigmoid", pair_scale=30.0, pair_bias=-8.0, train_pair_head=True))):
        for kind in ("paired", "groups"):
            L, cfg, sd, model, layers, lw = TC._model(dev, _Monkey, 0.25)
            img, cap, ig, cg = TC._batch(cfg, kind)
            model.train()
            tr = (L.LoRAPairTrainer if kw else L.LoRATrainer)(model, lr=1e-3, **kw)
            dg = lambda x: None if x is None else x.to(dev)
            tr.flat.zero_grad()
            loss, c_it, c_ti = tr.forward_backward_pairs(img.to(dev), cap.to(dev), dg(ig), dg(cg))
            grads = tr.flat.grads.clone()
            tr.optimizer_step()
            torch.cuda.synchronize()
            tag = f"{loss_name}_{kind}"
            arrays[f"{tag}_loss"] = loss.cpu().numpy()
            arrays[f"{tag}_hits"] = np.array([c_it.item(), -1 if c_ti is None else c_ti.item()], dtype=np.int32)
            arrays[f"{tag}_grads"] = grads.cpu().numpy()
            arrays[f"{tag}_params"] = tr.flat.params.cpu().numpy()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez(out, **arrays)
    print(f"dumped {len(arrays)} arrays of {root} to {out}")


def compare(a, b):
    x, y = np.load(a), np.load(b)
    assert sorted(x.files) == sorted(y.files), (x.files, y.files)
    same = 0
    for name in sorted(x.files):
        eq = x[name].shape == y[name].shape and x[name].tobytes() == y[name].tobytes()
        same += eq
        print(f"  {name}: bitwise={eq} shape={x[name].shape}")
    print(f"TOTAL: {same} of {len(x.files)} arrays bitwise equal")
    return same == len(x.files)


def digest(a):
    x = np.load(a)
    for name in sorted(x.files):
        print(f"{name} {x[name].dtype} {x[name].shape} {hashlib.sha256(x[name].tobytes()).hexdigest()}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--digest")
    args = ap.parse_args()
    if args.digest:
        digest(args.digest)
        sys.exit(0)
    if args.compare:
        sys.exit(0 if compare(*args.compare) else 1)
    dump(os.path.abspath(args.root), args.out)
