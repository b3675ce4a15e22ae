#!/usr/bin/env python3
"""Headline benchmark (BASELINE.json): images/sec of the ViT-B/32 forward + LoRA backward train step.

    python bench.py --gpus N --steps K --warmup W
    N > 1 either way: under a launcher (python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py
    --gpus N ...: RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the environment), or from a bare shell -- then this
    process, BEFORE it makes any GPU call, starts that same launcher as a child, relays rank 0's JSON line and
    exits with the child's status.

Workload (config.workload): cfg-2 of BASELINE.json -- ViT-B/32, rank-4 LoRA on q,k,v of all 12+12
blocks (weights = the reference's shipped lora_weights.pkl), 4 learnable text-prompt tokens, one
run_lora step (lora_train_vlp.py:956-1002): 403 captions through the text tower WITH grad, 256 images
through the image tower, 100*cos logits, cross entropy, backward into LoRA + prompt, AdamW.
Synthetic data (N(0,1) images, random captions, CLIP-init random backbone: no network), inputs resident
in HBM before the timed region.  One step = one such pass over one global batch of 256 images.

N > 1 is STRONG scaling (global batch fixed at 256, 256/N images per rank); the
text tower is class-sharded (ceil(403/N) captions per rank); collectives per step over RCCL: ONE
all_gather_into_tensor of the class-feature blocks, ONE reduce_scatter_tensor of their gradient and ONE all-reduce
of the flat 1.5 MB LoRA+prompt gradient buffer (clipfs/dist.py); under --full their per-step time is measured with HIP
events and reported (``collective_ms_per_step``).  ``--weak`` keeps 256 images per rank instead.

Rank 0 prints ONE JSON line.  A plain run sets up, warms up, times the K steps, writes ``--dump-outputs`` and prints
the headline fields; it runs nothing else.  ``--full`` adds every other measurement and check, each after the timed
region except the golden check (it needs the pristine adapters): ``top5_match`` (top-5 labels of the full-depth model
on the committed golden inputs, tests/golden/vitb32_full_step.npz), ``collective_ms_per_step`` (N > 1 or
--rccl-one-rank), ``roofline`` (dominant kernel = the fp32-MFMA GEMM; every GEMM launch of one extra, instrumented
step is bracketed by HIP events on its launch stream), ``variants`` (opt-in modes), ``forward_only`` (the
north-star's own target: image-tower forward at bs 256), ``cfg4`` (MTA test-time augmentation), ``cfg5`` (a short
ViT-L/14 fp16-mode leg) and ``cpu_baseline`` (the CPU oracle timed on the host cores on a bounded sample; N = 1
only).  The --no-* flags drop single legs of a --full run.
In the timed region the text tower runs on a side HIP stream next to the image tower (they are independent
until the logits); the instrumented roofline step serialises them so each GEMM's duration is its own.

``--dump-outputs DIR`` writes what the LAST timed step handed its caller -- loss_sum, correct, logits (rank 0's rows) and
the flat LoRA + prompt parameters after AdamW with the gradient it applied (``features`` under --forward-only) -- as
DIR/<name>.npy.  Inputs and weights come from fixed seeds, so two builds run with the same arguments can be compared
output for output.
"""
from __future__ import annotations

import argparse
import contextlib
import ctypes
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "jittor-clip-fewshot_amd"))
sys.path.insert(0, ROOT)

FP32_MFMA_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
# algorithmic GFLOP per unit (SURVEY.md section 8d / BASELINE.md section 2)
IMG_FWD, IMG_BWD = 8.8176 + 0.0221, 8.586 + 0.044
TXT_FWD, TXT_BWD = 5.9595 + 0.0227, 5.959 + 0.045
# Exact zeros the backward does not multiply: the heads read ONE row per sequence (class token / EOT token), so in the
# LAST block the gradient is zero in every other row until the attention mixes rows again -- its MLP and output-projection
# input-gradients (9 d^2 MACs per token) run on that one row (clipfs_tower_bwd_sparse).  Subtracted from the algorithmic
# count so that step_tflops prices only work an exact implementation has to do (GFLOP per image / caption):
IMG_BWD_ZERO = 9 * 768 * 768 * 2 * 49 / 1e9
TXT_BWD_ZERO = 9 * 512 * 512 * 2 * 76 / 1e9
# The forward has the same structure: after the last attention nothing but the class / EOT row is ever read, so the last
# block's output projection, LayerNorm 2 and MLP (the same 9 d^2 MACs per token) run on that row (clipfs_tower_fwd_rows):
IMG_FWD_ZERO, TXT_FWD_ZERO = IMG_BWD_ZERO, TXT_BWD_ZERO
# the same rows of ViT-L/14 (cfg-5: width 1024 / 257 tokens, text width 768 / 77 tokens), forward + backward together
L14_IMG_ZERO = 2 * 9 * 1024 * 1024 * 2 * 256 / 1e9
L14_TXT_ZERO = 2 * 9 * 768 * 768 * 2 * 76 / 1e9


# Environment knobs read by the library / host code (each once per process; the defaults ARE the product configuration).
# SCHEDULE knobs pick another kernel or launch geometry for the same arithmetic (results equal up to fp32 summation
# order); NUMERICS knobs change results and make a headline line meaningless: the bench refuses to print one.
NUMERICS_KNOBS = ("CLIPFS_GEMM_ABLATE",)


def env_overrides():
    knobs = {k: v for k, v in sorted(os.environ.items()) if k.startswith("CLIPFS_") and k != "CLIPFS_BENCH_REHEARSE"}
    if knobs:
        print("[bench] active CLIPFS_* overrides: " + " ".join(f"{k}={v}" for k, v in knobs.items()), file=sys.stderr, flush=True)
    else:
        print("[bench] no CLIPFS_* overrides set (product defaults)", file=sys.stderr, flush=True)
    bad = [k for k in knobs if k in NUMERICS_KNOBS and knobs[k] not in ("", "0")]
    if bad:
        raise SystemExit(f"bench.py: {', '.join(bad)} changes the arithmetic (timing-only diagnostic); refusing to emit a "
                         "benchmark line.  Unset it, or use scripts/ablate_gemm.py with an ablation build.")
    return knobs


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256, help="global image batch (strong scaling)")
    ap.add_argument("--classes", type=int, default=403)
    ap.add_argument("--weak", action="store_true", help="keep --batch images PER RANK (weak scaling)")
    ap.add_argument("--no-shard-text", action="store_true", help="replicate the text tower on every rank")
    ap.add_argument("--dropout", type=float, default=0.25, help="LoRA input dropout (reference default 0.25)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, run every other measurement and check: golden top-5, collective timing, "
                         "roofline step, opt-in variants, forward_only / cfg4 / cfg5 legs, CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-roofline", action="store_true", help="--full without the roofline step")
    ap.add_argument("--serial-towers", action="store_true",
                    help="run the text and image towers back to back on one stream (default: text tower on a side stream)")
    ap.add_argument("--model", choices=["b32", "l14"], default="b32",
                    help="b32: the headline ViT-B/32 cfg-2; l14: cfg-5 shapes (ViT-L/14, LoRA r=16, synthetic adapters)")
    ap.add_argument("--no-variants", action="store_true", help="--full without the opt-in-mode measurements")
    ap.add_argument("--precision", choices=["fp32", "bf16x3", "fp16"], default="fp32",
                    help="GEMM arithmetic of the towers: exact fp32 MFMA (default) or split-bf16 x3 (opt-in fast mode)")
    ap.add_argument("--trim-text", action="store_true",
                    help="opt-in: skip the text positions after the batch's last EOT (dead under the causal mask); "
                         "NOT the headline configuration")
    ap.add_argument("--forward-only", action="store_true", help="time the zero-grad image forward only (diagnostic)")
    ap.add_argument("--rccl-one-rank", action="store_true",
                    help="diagnostic at --gpus 1: an RCCL process group of ONE rank with the step's three collectives "
                         "issued anyway (their launch / stream cost on one card; no bytes cross xGMI)")
    ap.add_argument("--no-extras", action="store_true", help="--full without the forward_only / cfg4 / cfg5 legs")
    ap.add_argument("--cfg5-budget-s", type=float, default=150.0,
                    help="--full: skip the cfg-5 leg when the run has already taken this many seconds")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (rank 0)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(out_dir, arrays):
    """Writes ``arrays`` ({name: tensor}) as ``out_dir/<name>.npy`` in float32 (float64 where the tensor is float64).
    Each array gets an equal share of 64 MB; an array over its share is replaced by a fixed, seeded sample of its
    flattened elements (sorted indices, saved beside it as ``<name>_index.npy``), so two runs sample the same elements."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    share = DUMP_MAX_BYTES // (2 * len(arrays))  # room for a sample and its index per array
    written = []
    for name, t in arrays.items():
        a = t.detach().cpu().numpy()
        a = a.astype(np.float64 if a.dtype == np.float64 else np.float32)
        if a.nbytes > share:
            n = share // 8  # a float64 index per sampled element
            idx = np.sort(np.random.default_rng(0).choice(a.size, size=n, replace=False))
            np.save(os.path.join(out_dir, f"{name}_index.npy"), idx.astype(np.float64))
            written.append(f"{name}_index")
            a = a.reshape(-1)[idx]
        np.save(os.path.join(out_dir, f"{name}.npy"), a)
        written.append(name)
    return written


def self_launch(args) -> int:
    """``--gpus N`` from a bare shell: start the N ranks as a CHILD (torch.distributed.run), relay rank 0's JSON line.
    This process has made no GPU call (torch is not even imported yet), so nothing is re-exec'ed after GPU init."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__), *sys.argv[1:]]
    print("[bench] launching: " + " ".join(cmd), file=sys.stderr, flush=True)
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, env=env, text=True)
    line = None
    for ln in proc.stdout:
        t = ln.strip()
        if t.startswith("{") and '"metric"' in t:
            line = t
        else:
            sys.stderr.write(ln)
    rc = proc.wait()
    if rc != 0 or line is None:
        print(f"[bench] the {args.gpus}-rank child failed (rc={rc}, json={'yes' if line else 'no'})", file=sys.stderr, flush=True)
        return rc or 1
    print(line, flush=True)
    return 0


def build_trainer(dev, args, model_name=None, precision=None):
    import types
    import torch
    import lora_train_vlp as L
    from clipfs import synth
    from jclip.model import build_model
    model_name = model_name or args.model
    l14 = model_name == "l14"
    cfg = synth.VIT_L14 if l14 else synth.VIT_B32
    sd = synth.synth_state_dict(cfg, seed=1234)
    model = build_model(sd, device=dev)
    del sd
    largs = types.SimpleNamespace(encoder="both", position="all", backbone="ViT-L/14" if l14 else "ViT-B/32",
                                  params=["q", "k", "v"], r=16 if l14 else 4, alpha=1, dropout_rate=args.dropout)
    layers = L.apply_lora(largs, model)
    if l14:  # no shipped checkpoint for L/14: A ~ U(+-1/sqrt(in)), B ~ N(0, 0.02^2), seed 5
        lw = synth.synth_lora(cfg, 16, seed=5, vision_blocks=range(21))
        names = {"q": "q_proj", "k": "k_proj", "v": "v_proj"}
        with torch.no_grad():
            for i, layer in enumerate(layers):
                for p_ in "qkv":
                    m_ = getattr(layer, names[p_])
                    m_.w_lora_A.copy_(torch.from_numpy(lw[f"layer_{i}"][names[p_]]["w_lora_A"]))
                    m_.w_lora_B.copy_(torch.from_numpy(lw[f"layer_{i}"][names[p_]]["w_lora_B"]))
    else:
        import contextlib
        with contextlib.redirect_stdout(sys.stderr):  # load_lora prints like the reference; stdout carries ONE JSON line
            L.load_lora(largs, layers, os.path.join(ROOT, "tests", "golden", "lora_weights.pkl"))
    L.mark_only_lora_as_trainable(model)
    # 4 prompt tokens initialised from the embeddings of "a photo of a" (slow_pace.py:124-131)
    ids = torch.tensor([320, 1125, 539, 320], device=dev)
    ctx = torch.nn.Parameter(model.token_embedding.weight.data[ids].clone())
    model.train()
    tr = L.LoRATrainer(model, prompt_ctx=ctx, shard_text=not args.no_shard_text)
    tr.overlap_towers = not args.serial_towers
    model.engine.trim_text = args.trim_text
    model.engine.precision = precision or args.precision
    return model, tr, cfg


def golden_top5(model, tr, dev):
    """Top-5 labels of the (dropout-free) cfg-2 model on the committed golden inputs (8 images x 16 captions,
    tests/golden/vitb32_full_step.npz, written by the fp64 oracle): the metric's "top-5 match vs ref".  Must run before
    the first optimiser step (the golden holds the pristine shipped adapters)."""
    import numpy as np
    import torch
    from clipfs import engine, ops, synth
    path = os.path.join(ROOT, "tests", "golden", "vitb32_full_step.npz")
    if not os.path.exists(path):
        return None
    z = np.load(path)
    B, Cn = z["eval_logits"].shape
    img = synth.synth_images(B, 224, seed=0).to(dev)
    cap = synth.synth_captions(Cn, 77, synth.VIT_B32.vocab_size, seed=1).to(dev)
    model.eval()
    with torch.no_grad():
        fi = ops.l2norm_fwd(model.encode_image(img))
        ft = ops.l2norm_fwd(engine.encode_text(model, cap, tr.prompt_ctx))
        logits = ops.gemm_nt(fi, ft, alpha=100.0)
        top5 = ops.topk(logits, 5).cpu().numpy()
    model.train()
    err = float(np.abs(logits.cpu().numpy() - z["eval_logits"]).max())
    return {"top5_match": bool(np.array_equal(top5, z["eval_top5"])), "max_abs_logit_err": round(err, 7),
            "tolerance": 1e-3, "golden": "tests/golden/vitb32_full_step.npz (fp64 oracle; 8 images x 16 captions, full-depth "
                                        "ViT-B/32 + shipped LoRA + prompt tokens)"}


def host_cores() -> int:
    """CPU share of this process: the affinity mask, capped at the GPU box's per-GPU share of 16."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(n, 16))


def cpu_model() -> str:
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(full_step_budget_s=45.0):
    """The CPU oracle (oracle/clip_oracle.py, fp32 PyTorch-CPU restatement) on the host cores:
    B = 8 images + 13 captions (the 256:403 ratio), forward and forward + LoRA backward, 2 warm-up + 5 timed
    iterations each, median; then ONE full cfg-2 step (256 images + 403 captions) when the B = 8 time predicts it
    fits the budget, else the B = 8 figure stands for it (the work is linear in B)."""
    import torch
    from clipfs import safe_pkl, synth
    from oracle import clip_oracle as O
    cfg = synth.VIT_B32
    cores = host_cores()
    torch.set_num_threads(cores)
    sd = synth.synth_state_dict(cfg, seed=1234)
    ck = safe_pkl.load(os.path.join(ROOT, "tests", "golden", "lora_weights.pkl"))
    tl, vl = O.split_lora_checkpoint(ck["weights"], "both", "all", "ViT-B/32", dtype=torch.float32)
    params = [t for blk in list(tl.values()) + list(vl.values()) for ab in blk.values() for t in ab.values()]
    for t in params:
        t.requires_grad_()

    def run(B, Cn, backward):
        img = synth.synth_images(B, 224, seed=0)
        cap = synth.synth_captions(Cn, 77, cfg.vocab_size, seed=1)
        tgt = synth.synth_labels(B, Cn, seed=2)
        t0 = time.time()
        if backward:
            for t in params:
                t.grad = None
            loss, _ = O.train_step_loss(sd, img, cap, tgt, tl, vl, 0.5)
            loss.backward()
        else:
            with torch.no_grad():
                O.train_step_loss(sd, img, cap, tgt, tl, vl, 0.5)
        return time.time() - t0

    def median(B, Cn, backward, warm=2, timed=5):
        ts = [run(B, Cn, backward) for _ in range(warm + timed)][warm:]
        return sorted(ts)[len(ts) // 2]

    B, Cn = 8, 13
    t_fwd = median(B, Cn, False)
    t_step = median(B, Cn, True)
    print(f"[bench] cpu baseline B=8: fwd {t_fwd:.2f} s, fwd+bwd {t_step:.2f} s", file=sys.stderr, flush=True)
    out = {"value": round(B / t_step, 3), "unit": "images/s", "cores": cores, "cpu_model": cpu_model(), "kind": "port",
           "forward_images_per_s": round(B / t_fwd, 3),
           "sample": f"oracle fp32 (PyTorch-CPU restatement, NOT Jittor: Jittor is not installable offline), "
                     f"{B} images + {Cn} captions, forward and forward+LoRA-backward, median of 5 after 2 warm-ups"}
    predicted = t_step * 256 / B
    if predicted <= full_step_budget_s:
        t_full = run(256, 403, True)
        out["b256_step"] = {"images_per_s": round(256 / t_full, 3), "seconds": round(t_full, 2),
                            "sample": "ONE full cfg-2 step on the CPU: 256 images + 403 captions forward+LoRA-backward"}
        print(f"[bench] cpu baseline B=256 step: {t_full:.1f} s", file=sys.stderr, flush=True)
    else:
        out["b256_step"] = {"images_per_s": round(B / t_step, 3), "seconds": round(predicted, 1),
                            "sample": "extrapolated from B = 8 (work is linear in the batch); not run: over the time budget"}
    return out


def gemm_traffic(lib, args):
    """HBM-side traffic per launch of the dominant GEMM from the committed rocprofv3 --pmc passes (the counters cannot be
    read from inside this process).  The file carries the source stamp of the GEMM it was measured on; a mismatch with the
    loaded library means the figure is stale -> traffic is reported as null."""
    if args.precision != "fp32" or args.model != "b32":
        return None, "no PMC passes for this mode"
    stamp = lib.clipfs_gemm_source_stamp().decode()
    prof = os.path.join(ROOT, "profiles")
    rounds = sorted(d for d in os.listdir(prof) if os.path.isfile(os.path.join(prof, d, "gemm_traffic.json"))) \
        if os.path.isdir(prof) else []
    for d in reversed(rounds):
        with open(os.path.join(prof, d, "gemm_traffic.json")) as f:
            j = json.load(f)
        if j.get("gemm_source_stamp") == stamp:
            return j.get("traffic_bytes_per_launch"), (
                f"profiles/{d}/gemm_traffic.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over this command, FETCH x2 "
                f"per the gfx950 note; L2-side counters: Infinity-Cache hits included; measured on GEMM source {stamp})")
    return None, f"no committed PMC pass matches the loaded GEMM (source stamp {stamp}): stale figures are not reported"


def main():
    args = parse()
    t_start = time.time()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_launch(args))
    knobs = env_overrides() if int(os.environ.get("RANK", "0")) == 0 else {}
    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (the HIP engine has no CPU fallback)")
    # CLIPFS_BENCH_REHEARSE=1: run the N-rank code path on a box with fewer GPUs than ranks (ranks share cards, gloo
    # instead of RCCL, which refuses two ranks on one device).  A correctness rehearsal only -- never a measurement.
    rehearse = os.environ.get("CLIPFS_BENCH_REHEARSE") == "1"
    if rehearse:
        local_rank %= torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if rehearse:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            with stdout_to_stderr():  # RCCL prints a version banner on STDOUT when the communicator is created
                dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
                dist.all_reduce(torch.zeros(1, device=dev))
                torch.cuda.synchronize()
    elif args.rccl_one_rank:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(29500 + os.getpid() % 2000))
        with stdout_to_stderr():
            dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
            dist.all_reduce(torch.zeros(1, device=dev))
            torch.cuda.synchronize()

    from clipfs import _lib, dist as D, synth
    # ranks of the communicator the first collective above actually completed on (not the launcher's WORLD_SIZE)
    live_ranks = dist.get_world_size() if dist.is_initialized() else 0
    if args.rccl_one_rank and world == 1:
        D.FORCE_COLLECTIVES = True
    lib = _lib.load()
    model, tr, cfg = build_trainer(dev, args)
    # eval mode draws no dropout seed, so the timed steps see the same seeds with or without this check
    top5 = golden_top5(model, tr, dev) if (args.full and args.model == "b32" and rank == 0) else None
    gb = args.batch * world if args.weak else args.batch
    lo, hi = D.shard_bounds(gb, rank, world)
    images = synth.synth_images(gb, 224, seed=0)[lo:hi].contiguous().to(dev)
    labels = synth.synth_labels(gb, 374, seed=2)[lo:hi].contiguous().to(dev)
    captions = synth.synth_captions(args.classes, 77, cfg.vocab_size, seed=1).to(dev)
    # caption rows 1..4 are the learnable prompt slots; keep EOT after them (synthetic captions have len >= 6)

    last = {}  # what the most recent step() returned to its caller (--dump-outputs)

    def step():
        if args.forward_only:
            with torch.no_grad():
                last["features"], _ = model.engine.vit_forward(images, False)
            return
        tr.flat.zero_grad()
        last["loss_sum"], last["correct"], last["logits"] = tr.forward_backward(images, captions, labels, 1, gb,
                                                                                 row_offset=lo)
        tr.optimizer_step()

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    t_setup = time.time() - t_start
    for i in range(args.warmup):
        step()
        if rank == 0:
            torch.cuda.synchronize()
            print(f"[bench] warmup step {i} done", file=sys.stderr, flush=True)
    barrier()
    if rank == 0:
        print(f"[bench] set up in {t_setup:.1f} s, {args.warmup} warm-up steps in {time.time() - t_start - t_setup:.1f} s",
              file=sys.stderr, flush=True)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    t_issue = time.perf_counter() - t0  # host time to enqueue the K steps (== dt when the host, not the GPU, is the limit)
    barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        tmax = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = tmax.item()
    ms = dt / args.steps * 1e3
    value = gb * args.steps / dt

    # ---- the last timed step's results, before any later leg steps the trainer again ----
    if args.dump_outputs and rank == 0:
        arrays = dict(last)
        if not args.forward_only:  # the optimiser's result: flat LoRA + prompt parameters and the gradient it applied
            arrays.update(params=tr.flat.params, grads=tr.flat.grads)
        names = dump_outputs(args.dump_outputs, arrays)
        print(f"[bench] outputs of the last timed step written to {args.dump_outputs}: {', '.join(names)}",
              file=sys.stderr, flush=True)

    # ---- collectives: three more steps with every collective bracketed by HIP events on its launch stream ----
    coll = None
    if args.full and (world > 1 or args.rccl_one_rank) and not args.forward_only:
        tr.time_collectives = True
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        tr.time_collectives = False
        times = tr.collective_times_ms()
        per = {k: round(sum(v) / len(v), 4) for k, v in times.items()}
        tot = torch.tensor([sum(per.values())], device=dev, dtype=torch.float64)
        dist.all_reduce(tot, op=dist.ReduceOp.MAX)
        coll = {"per_collective_ms": per, "total_ms_per_step_max_rank": round(tot.item(), 4),
                "note": "HIP events around each collective on rank 0's launch stream (includes waiting for the slowest rank)"}
    barrier()

    # ---- roofline leg: one more step with every GEMM launch bracketed by HIP events on its stream ----
    roof = None
    if args.full and not args.no_roofline:
        overlap = tr.overlap_towers
        tr.overlap_towers = False  # per-kernel durations are only meaningful when nothing else shares the GPU
        lib.clipfs_gemm_timing(1)
        step()
        torch.cuda.synchronize()
        lib.clipfs_gemm_timing(0)
        tr.overlap_towers = overlap
        roof = collect_roofline(lib, args, args.precision)
    barrier()

    # ---- opt-in modes next to the headline (same step, same inputs; never the headline `value`) ----
    variants = None
    if args.full and world == 1 and not args.no_variants and not args.forward_only and args.model == "b32" and \
            args.precision == "fp32" and not args.trim_text:
        variants = {}
        # the same step with every block dense in both directions (the one-row-per-sequence gradient scattered into zeros)
        model.engine.sparse_backward = False
        step()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        vdt = (time.perf_counter() - t1) / 3
        model.engine.sparse_backward = True
        variants["dense_last_block"] = {
            "value": round(gb / vdt, 2), "unit": "images/s", "ms_per_step": round(vdt * 1e3, 3),
            "note": "identical features and gradients; the last block's out-proj / LayerNorm 2 / MLP and their input-gradients "
                    "computed for all 12 800 + 31 031 rows although only the 256 class-token + 403 EOT rows are read / non-zero "
                    "(what round 1 measured; algorithmic 9.303 TFLOP per step)"}
        for name, trim, prec, note in (
                ("trim_text", True, "fp32", "exact fp32; text tower evaluated only up to the last EOT of the batch (positions "
                                            "after a caption's EOT cannot reach its feature under the causal mask)"),
                ("bf16x3", False, "bf16x3", "tower GEMMs as split-bf16 (3 bf16 MFMA products, fp32 accumulate); logits within "
                                            "~3e-4 of fp32, inside the 1e-3 budget"),
                ("bf16x3+trim_text", True, "bf16x3", "both")):
            model.engine.trim_text, model.engine.precision = trim, prec
            step()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(3):
                step()
            torch.cuda.synchronize()
            vdt = (time.perf_counter() - t1) / 3
            variants[name] = {"value": round(gb / vdt, 2), "unit": "images/s", "ms_per_step": round(vdt * 1e3, 3), "note": note}
        model.engine.trim_text, model.engine.precision = args.trim_text, args.precision

    # ---- the north-star's own target: image-tower forward at bs 256 (>= 40 % of the MFMA roofline) ----
    fwd_only = None
    extras = args.full and world == 1 and not args.no_extras and not args.forward_only and args.model == "b32" and \
        args.precision == "fp32" and not args.trim_text
    if extras:
        with torch.no_grad():
            for _ in range(3):
                model.engine.vit_forward(images, False)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(10):
                model.engine.vit_forward(images, False)
            torch.cuda.synchronize()
        fdt = (time.perf_counter() - t1) / 10
        ftf = gb * (IMG_FWD - (IMG_FWD_ZERO if model.engine.sparse_backward else 0)) / 1e3 / fdt
        fwd_only = {"value": round(gb / fdt, 1), "unit": "images/s", "ms": round(fdt * 1e3, 3), "batch": gb,
                    "tflops": round(ftf, 2), "frac_of_fp32_mfma_peak": round(ftf / FP32_MFMA_PEAK_TFLOPS, 4),
                    "workload": "ViT-B/32 image tower forward (eval, LoRA applied, no dropout), 10 passes after 3 warm-ups; the last "
                                "block after its attention on the class-token rows only (8.319 algorithmic GFLOP per image)",
                    "north_star_target": ">= 0.40 of the MFMA roofline"}

    # ---- cfg-4 leg: MTA test-time augmentation, 8 source images x (1 + 64) views (ood.py:857-883) ----
    cfg4 = None
    if extras:
        cfg4 = cfg4_leg(dev, model, captions)

    # ---- cfg-5 leg: ViT-L/14, rank-16 LoRA, fp16 storage mode, 128 images (one rank's share of bs 1024) + 403 captions ----
    cfg5 = None
    if extras:
        if time.time() - t_start > args.cfg5_budget_s:
            cfg5 = {"skipped": f"run already took {time.time() - t_start:.0f} s (budget {args.cfg5_budget_s:.0f} s)"}
        else:
            del images
            model = tr = None
            torch.cuda.empty_cache()
            cfg5 = cfg5_leg(dev, args, lib)

    if rank == 0:
        n_img_local = hi - lo
        if args.model == "l14":  # 162.03 (+0.303 LoRA) per image, 13.30 per caption; dgrad ~= forward
            dense_bwd = os.environ.get("CLIPFS_DENSE_BWD", "0") not in ("", "0")
            step_tflop = (gb * (2 * (162.03 + 0.303) - (0 if dense_bwd else L14_IMG_ZERO)) +
                          args.classes * (2 * 13.30 - (0 if dense_bwd else L14_TXT_ZERO))) / 1e3
        elif args.forward_only:
            dense_bwd = os.environ.get("CLIPFS_DENSE_BWD", "0") not in ("", "0")
            step_tflop = gb * (IMG_FWD - (0 if dense_bwd else IMG_FWD_ZERO)) / 1e3
        else:
            dense_bwd = os.environ.get("CLIPFS_DENSE_BWD", "0") not in ("", "0")
            step_tflop = (gb * (IMG_FWD + IMG_BWD - (0 if dense_bwd else IMG_FWD_ZERO + IMG_BWD_ZERO)) +
                          args.classes * (TXT_FWD + TXT_BWD - (0 if dense_bwd else TXT_FWD_ZERO + TXT_BWD_ZERO))) / 1e3
        backend = D.backend_name()
        out = {
            "metric": "images/sec ViT-B/32 fwd+LoRA-bwd bs=256" if args.model == "b32" else
                      "images/sec ViT-L/14 fwd+LoRA-bwd (cfg-5 shapes)", "value": round(value, 2), "unit": "images/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 3),
            "host_issue_ms_per_step": round(t_issue / args.steps * 1e3, 3),
            "higher_is_better": True, "scaling": "weak" if args.weak else "strong", "vs_baseline": None,
            "dtype": {"fp32": "f32", "bf16x3": "f32 (tower GEMMs as split-bf16 x3 MFMA, fp32 accumulate)", "fp16": "f16 operands in the tower GEMMs, fp32 accumulate"}[args.precision], "data": "synthetic",
            "config": {"workload": ("ViT-B/32 image tower forward only (diagnostic)" if args.forward_only else
                                    "cfg-5 shapes: ViT-L/14 + rank-16 LoRA(q,k,v; 12 text + 21 vision blocks, synthetic adapters) + 4 "
                                    "text-prompt tokens; run_lora train step, fp16 storage mode when --precision fp16"
                                    if args.model == "l14" else
                                    "cfg-2: ViT-B/32 + rank-4 LoRA(q,k,v; 12 text + 12 vision blocks; shipped "
                                    "lora_weights.pkl) + 4 text-prompt tokens; run_lora train step = text tower "
                                    "fwd+bwd on 403 captions + image tower fwd+bwd + 100*cos CE + AdamW"),
                       "global_batch": gb, "images_per_rank": n_img_local, "captions": args.classes,
                       "last_block": "dense (CLIPFS_DENSE_BWD=1)" if os.environ.get("CLIPFS_DENSE_BWD", "0") not in ("", "0")
                       else "after its attention, forward and backward on one row per sequence (the class / EOT row: the only "
                            "row read, the only row with gradient; exact -- `variants.dense_last_block` of --full is the all-rows step)",
                       "lora_dropout": args.dropout, "tower_streams": 1 if args.serial_towers else 2, "text_positions": "trimmed-to-last-EOT" if args.trim_text else 77, "parallelism": f"dp{world}" + ("" if args.no_shard_text or world == 1 else "+class-sharded-text")},
            "algorithmic_tflop_per_step": round(step_tflop, 3),
            "step_tflops": round(step_tflop / (ms * 1e-3), 2),
            "step_frac_of_fp32_mfma_peak": round(step_tflop / (ms * 1e-3) / (FP32_MFMA_PEAK_TFLOPS * world), 4),
            "backend": backend,
            "rccl_ranks": live_ranks if backend == "nccl" else 0,
            "collectives_per_step": tr.collectives_per_step if tr is not None else 0,
        }
        if rehearse:
            out["rehearsal"] = "CLIPFS_BENCH_REHEARSE=1: ranks share GPUs over gloo -- a code-path rehearsal, NOT a measurement"
        if coll:
            out["collective_ms_per_step"] = coll
        if top5:
            out.update(top5_match=top5["top5_match"], top5=top5)
        if roof:
            out["roofline"] = roof
        if fwd_only:
            out["forward_only"] = fwd_only
        if cfg4:
            out["cfg4"] = cfg4
        if cfg5:
            out["cfg5"] = cfg5
        if variants:
            out["variants"] = variants
        if args.full and world == 1 and not args.no_cpu_baseline and not args.forward_only:
            out["cpu_baseline"] = cpu_baseline()
        if knobs:
            out["env_overrides"] = knobs
        print(json.dumps(out), flush=True)
    if dist.is_initialized():  # world > 1, or the one-rank RCCL group of --rccl-one-rank
        dist.barrier()
        dist.destroy_process_group()


@contextlib.contextmanager
def stdout_to_stderr():
    """File-descriptor level: native libraries (RCCL's start-up banner) write to fd 1 directly, and stdout must carry
    the JSON line alone."""
    sys.stdout.flush()
    saved = os.dup(1)
    try:
        os.dup2(2, 1)
        yield
    finally:
        sys.stdout.flush()
        os.dup2(saved, 1)
        os.close(saved)


def collect_roofline(lib, args, precision):
    tms, tfl, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
    lib.clipfs_gemm_timing_collect(ctypes.byref(tms), ctypes.byref(tfl), ctypes.byref(n))
    if n.value <= 0 or tms.value <= 0:
        return None
    ach = tfl.value / (tms.value * 1e-3) / 1e12
    # achieved counts ALGORITHMIC FLOPs (2MNK); the opt-in 16-bit modes are priced against the dense 16-bit
    # MFMA peak divided by the products they spend per algorithmic multiply (3 for split-bf16, 1 for f16)
    kname, peak = {
        "fp32": ("gemm_nt_kernel<64,128,3> (v_mfma_f32_32x32x2_f32, global_load_lds staging)", FP32_MFMA_PEAK_TFLOPS),
        "bf16x3": ("gemm_bf16x3_kernel<.,.,2> (3 x v_mfma_f32_32x32x16_bf16 per operand pair)", 2500.0 / 3),
        "fp16": ("gemm_f16_ph_kernel 256x256x64, four quadrant phases per K-tile (v_mfma_f32_16x16x32_f16; "
                 "both operands f16 via global_load_lds) + gemm_f16_kernel<64,128,2> on the leftover rows beside it; peak = the "
                 "2.5 PFLOP/s spec, the board holds 1.75 GHz of 2.4 under this load (1.4 kW cap)", 2500.0),
    }[precision]
    traffic, tsrc = gemm_traffic(lib, args) if precision == args.precision else (None, "not collected for this leg")
    return {"bound": "mfma", "kernel": kname,
            "achieved": round(ach, 2), "peak": round(peak, 1), "unit": "TFLOP/s",
            "frac": round(ach / peak, 4), "traffic": traffic, "traffic_unit": "bytes/launch", "traffic_source": tsrc,
            "algorithmic_bytes_per_launch": round(lib.clipfs_gemm_timing_last_bytes() / n.value),
            "launches_per_step": n.value, "avg_launch_us": round(tms.value * 1e3 / n.value, 2),
            "gflop_per_launch": round(tfl.value / n.value / 1e9, 3),
            "gemm_ms_per_step": round(tms.value, 3)}


def cfg4_leg(dev, model, captions, n_img=8, n_crops=64, passes=5):
    """BASELINE.json configs[3] on one GPU: per source image 1 centre view + 64 random crops generated ON THE GPU from
    the uint8 image (csrc/views.hip; the reference's CPU/PIL worker loop ood.py:946-958), ONE image-tower forward over
    all n_img * 65 views, L2-normalise, ONE mta_kernel launch (a workgroup per image; solve_mta, ood.py:742-811 ->
    lora_train_vlp.py:742-811), top-5 labels + base/new split (ood.py:873-883).  Correctness: the MTA kernel on the
    committed fixture (tests/golden/mta_v65.npz, fp64 oracle) -- top-5 identical, logits within 1e-3."""
    import numpy as np
    import torch
    import ood
    import tta
    from clipfs import ops
    V = 1 + n_crops
    t0 = time.time()
    was_training = model.training
    model.eval()
    rng = np.random.RandomState(7)
    srcs = [torch.from_numpy(rng.randint(0, 256, (375, 500, 3), dtype=np.uint8)).to(dev) for _ in range(n_img)]
    with torch.no_grad():
        text = ops.l2norm_fwd(model.encode_text(captions))

        def one_pass(seed0):
            views = torch.stack([tta.make_tta_views(srcs[i], n_crops, seed=seed0 + i) for i in range(n_img)])
            return ood.score_views(model, views, text)

        for w in range(2):
            one_pass(100 * w)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for it in range(passes):
            top5, is_base, logits = one_pass(1000 * (it + 1))
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t1) / passes
        # the same groups as a pipeline (views of group g + 1 and MTA of group g - 1 on the side stream under the tower pass of
        # group g: ood.score_stream; the reference overlaps these stages with DataLoader workers, ood.py:946-958)
        groups = 2 * passes
        ood.score_stream(model, srcs * 2, text, n_crops=n_crops, images_per_pass=n_img, seed=100)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        s_top5, _, s_logits = ood.score_stream(model, srcs * groups, text, n_crops=n_crops, images_per_pass=n_img, seed=1000)
        torch.cuda.synchronize()
        dt_stream = (time.perf_counter() - t2) / groups
        assert s_top5.shape == (n_img * groups, 5) and bool(torch.isfinite(s_logits).all())
        # the pieces, each timed alone with HIP events on the current stream
        def timed(fn, n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            fn()
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / n
        views = torch.stack([tta.make_tta_views(srcs[i], n_crops, seed=i) for i in range(n_img)])
        feats = ops.l2norm_fwd(model.encode_image(views.reshape(n_img * V, 3, 224, 224))).reshape(n_img, V, -1).contiguous()
        mta_ms = timed(lambda: ops.mta(feats, text), 10)
        view_ms = timed(lambda: tta.make_tta_views(srcs[0], n_crops, seed=3), 10)
        tower_ms = timed(lambda: model.encode_image(views.reshape(n_img * V, 3, 224, 224)), 3)
        assert top5.shape == (n_img, 5) and is_base.shape == (n_img,) and bool(torch.isfinite(logits).all())
        out = {"workload": f"cfg-4 on ONE GPU: {n_img} source images (500 x 375 uint8) x (1 centre + {n_crops} random-crop) views "
                           "generated on the GPU, ViT-B/32 + LoRA image-tower forward over all views, MTA (one workgroup per "
                           f"image, C = {text.shape[0]}), top-5 + base/new; {passes} passes after 2 warm-ups",
               "source_images_per_s": round(n_img / dt_stream, 2), "views_per_s": round(n_img * V / dt_stream, 1),
               "ms_per_pass": round(dt_stream * 1e3, 3), "groups": groups,
               "schedule": "ood.score_stream: view generation of the next group and MTA + top-5 of the previous one on the "
                           f"process's high-priority side stream under the tower pass of the current group of {n_img} images "
                           "(results identical to the one-stream loop, tests/test_tta_gpu.py); the tower pass alone is the floor",
               "one_stream": {"source_images_per_s": round(n_img / dt, 2), "views_per_s": round(n_img * V / dt, 1),
                              "ms_per_pass": round(dt * 1e3, 3), "passes": passes}, "mta_ms_per_image": round(mta_ms / n_img, 4),
               "mta_kernel_ms": round(mta_ms, 4), "view_generation_ms_per_image": round(view_ms, 4),
               "tower_forward_ms": round(tower_ms, 3), "base_fraction": round(float(is_base.float().mean().item()), 3)}
        gpath = os.path.join(ROOT, "tests", "golden", "mta_v65.npz")
        if os.path.exists(gpath):
            z = np.load(gpath)
            f = torch.from_numpy(z["feats"]).to(dev).unsqueeze(0).repeat(n_img, 1, 1)
            tt = torch.from_numpy(z["text"]).to(dev)
            _, gl = ops.mta(f, tt)
            g5 = ops.topk(gl, 5).cpu().numpy()
            want = z["logits64"] if "logits64" in z.files else z["logits"]
            out["top5_match"] = bool(all(np.array_equal(g5[i], z["top5"][0]) for i in range(n_img)))
            out["max_abs_logit_err"] = round(float(np.abs(gl.cpu().numpy() - want[0]).max()), 7)
            out["tolerance"] = 1e-3
            out["golden"] = "tests/golden/mta_v65.npz (fp64 oracle of solve_mta on 65 views x 403 classes)"
    if was_training:
        model.train()
    print(f"[bench] cfg4 leg: {dt_stream * 1e3:.1f} ms/pass pipelined (ood.score_stream), {dt * 1e3:.1f} on one stream ({time.time() - t0:.0f} s)",
          file=sys.stderr, flush=True)
    return out


def cfg5_golden_check(dev, args):
    """Full-depth correctness of the fp16 storage mode: the committed ViT-L/14 fixture (tests/golden/vitl14_full_step.npz,
    fp64 oracle, 24 + 12 blocks, r = 16 on 21 + 12 blocks, 4 images x 8 captions) evaluated by THIS process's fp16-mode
    engine: dropout-free logits (100 x cosine) and top-5."""
    import numpy as np
    import torch
    from clipfs import engine, ops, synth
    path = os.path.join(ROOT, "tests", "golden", "vitl14_full_step.npz")
    if not os.path.exists(path):
        return None
    z = np.load(path)
    model, tr, cfg = build_trainer(dev, args, model_name="l14", precision="fp16")
    B, Cn = z["eval_logits"].shape
    img = synth.synth_images(B, 224, seed=0).to(dev)
    cap = synth.synth_captions(Cn, 77, cfg.vocab_size, seed=1).to(dev)
    model.eval()
    with torch.no_grad():
        fi = ops.l2norm_fwd(model.encode_image(img))
        ft = ops.l2norm_fwd(engine.encode_text(model, cap, tr.prompt_ctx))
        logits = ops.gemm_nt(fi, ft, alpha=100.0)
        top5 = ops.topk(logits, 5).cpu().numpy()
    model.train()
    err = float(np.abs(logits.cpu().numpy() - z["eval_logits"]).max())
    rows = int(sum(np.array_equal(top5[i], z["eval_top5"][i]) for i in range(B)))
    return model, tr, cfg, {
        "top5_match": rows == B, "top5_rows_matching": rows, "rows": B, "top1_match": bool((top5[:, 0] == z["eval_top5"][:, 0]).all()),
        "max_abs_logit_err": round(err, 6), "tolerance": 2e-2,
        "golden": "tests/golden/vitl14_full_step.npz (fp64 oracle; full-depth ViT-L/14, 4 images x 8 captions; the fp16 storage "
                  "mode's stated budget is 2e-2 on 100 x cosine logits, tests/test_golden_gpu.py)"}


def cfg5_leg(dev, args, lib):
    """BASELINE.json configs[4] on one rank's share: ViT-L/14, rank-16 LoRA, fp16 storage mode (f16 x f16 MFMA GEMMs,
    f16 MFMA attention, fp32 accumulate / residual stream), 128 images + 403 captions per step."""
    import torch
    from clipfs import synth
    B = 128
    t0 = time.time()
    chk = cfg5_golden_check(dev, args)  # before the first optimiser step: the fixture holds the pristine adapters
    if chk is None:
        model, tr, cfg = build_trainer(dev, args, model_name="l14", precision="fp16")
        top5 = None
    else:
        model, tr, cfg, top5 = chk
    images = synth.synth_images(B, 224, seed=0).to(dev)
    labels = synth.synth_labels(B, 374, seed=2).to(dev)
    captions = synth.synth_captions(403, 77, cfg.vocab_size, seed=1).to(dev)

    def step():
        tr.flat.zero_grad()
        tr.forward_backward(images, captions, labels, 1, B)
        tr.optimizer_step()

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    n = 6
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t1) / n
    tr.overlap_towers = False
    lib.clipfs_gemm_timing(1)
    step()
    torch.cuda.synchronize()
    lib.clipfs_gemm_timing(0)
    roof = collect_roofline(lib, args, "fp16")
    step_tflop = (B * (2 * (162.03 + 0.303) - L14_IMG_ZERO) + 403 * (2 * 13.30 - L14_TXT_ZERO)) / 1e3
    print(f"[bench] cfg5 leg: {dt * 1e3:.1f} ms/step ({time.time() - t0:.0f} s incl. model build)", file=sys.stderr, flush=True)
    return {"workload": "cfg-5 shapes on ONE GPU: ViT-L/14 + rank-16 LoRA (synthetic adapters), fp16 storage mode, 128 images "
                        "(one rank's share of bs 1024) + 403 captions, train step; 6 steps after 3 warm-ups",
            "value": round(B / dt, 1), "unit": "images/s", "ms_per_step": round(dt * 1e3, 2),
            "step_tflops": round(step_tflop / dt, 1), "step_frac_of_f16_mfma_peak": round(step_tflop / dt / 2500.0, 4),
            "top5_match": None if top5 is None else top5["top5_match"],
            "max_abs_logit_err": None if top5 is None else top5["max_abs_logit_err"], "top5": top5,
            "gemm": roof}


if __name__ == "__main__":
    main()
