"""The one-wave-per-row adapter kernels (csrc/lora.hip) at two of the towers' own widths, where the default dispatch
never runs them: one child process under CLIPFS_LORA_MFMA=0 (the aid is read once per process) runs the
down-projection and the backward at

  rows 333, width 512, r 16, nseg 3, p 0.25        rows 130, width 1024, r 4, nseg 1, p 0

against the fp64 restatement of test_kernels_gpu.py::test_lora_down_and_bwd with the oracle's Philox masks, its generators
and its budgets: 2e-5 for t, 2e-4 for dA, dB and dx.  An fp32 emulation of this family's summation order (sequential
over a slice's rows, then over the slices) gives 9e-6 (dB) and 1.7e-5 (dA) at the first shape, 4e-6 and 1.1e-5 at the
second: more than ten times inside the budgets.  Measured on an MI355X: t 5.2e-7 | 3.2e-7, dA 1.8e-5 | 1.2e-5,
dB 8.1e-6 | 4.0e-6, dx 3.9e-7 | 1.2e-7.  The child prints the family clipfs_lora_plan names for each shape; the
parent asserts that it was "row"."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(333, 512, 16, 3, 0.25), (130, 1024, 4, 1, 0.0)]
T_TOL, GRAD_TOL = 2e-5, 2e-4
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _rand(*shape, seed=0, scale=1.0):
    import torch
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def _child():
    """under CLIPFS_LORA_MFMA=0: one JSON line per shape with the plan's family and the worst error of each output"""
    sys.path[:0] = [os.path.join(ROOT, "jittor-clip-fewshot_amd"), ROOT]
    import torch
    from clipfs import _lib, ops
    from oracle import clip_oracle as O
    dev = torch.device("cuda:0")
    seed, sb, scale = 0x1234ABCD5, 7, 0.5
    for rows, width, r, nseg, p in SHAPES:
        x = _rand(rows, width, seed=1)
        A = _rand(nseg * r, width, seed=2, scale=width ** -0.5).requires_grad_()
        Bm = _rand(nseg * width, r, seed=3, scale=0.1).requires_grad_()
        xs = x.clone().requires_grad_()
        ts, parts = [], []
        for s in range(nseg):
            m = torch.ones(rows, width, dtype=torch.float64)
            if p > 0:
                m = torch.from_numpy(O.dropout_keep_mask(seed, sb + s, rows, width, p)).double() / (1 - p)
            ts.append((xs * m) @ A[s * r:(s + 1) * r].t())
            parts.append(scale * ts[-1] @ Bm[s * width:(s + 1) * width].t())
        dy = _rand(rows, nseg * width, seed=4)
        torch.cat(parts, dim=1).backward(dy)
        D = lambda t: t.detach().float().to(dev)
        gseed = seed if p > 0 else 0
        t_gpu = ops.lora_down(D(x), D(A), r, nseg, p=p, seed=gseed, stream_base=sb)
        dA, dB = torch.zeros(nseg * r, width, device=dev), torch.zeros(nseg * width, r, device=dev)
        dx = torch.zeros(rows, width, device=dev)
        ops.lora_bwd(D(dy), D(x), t_gpu, D(A), D(Bm), dA, dB, dx=dx, scale=scale, p=p, seed=gseed, stream_base=sb)
        err = lambda got, want: (got.double().cpu() - want.detach()).abs().max().item()
        print("RESULT " + json.dumps(dict(
            shape=[rows, width, r, nseg], down=_lib.lora_plan("down", rows, width, width, r, nseg)["family"],
            bwd=_lib.lora_plan("bwd", rows, width, width, r, nseg)["family"], t=err(t_gpu, torch.cat(ts, dim=1)),
            dA=err(dA, A.grad), dB=err(dB, Bm.grad), dx=err(dx, xs.grad))), flush=True)


def test_row_family_at_tower_widths():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    env = dict(os.environ, CLIPFS_LORA_MFMA="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = [json.loads(l[7:]) for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    print(r.stdout)
    assert [g["shape"] for g in got] == [list(s[:4]) for s in SHAPES]
    for g in got:
        assert g["down"] == g["bwd"] == "row", g
        assert g["t"] <= T_TOL, g
        assert max(g["dA"], g["dB"], g["dx"]) <= GRAD_TOL, g


if __name__ == "__main__":
    _child()
