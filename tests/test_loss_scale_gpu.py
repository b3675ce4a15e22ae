"""Loss scaling on the GPU: the non-finite check and the scaler's decision against a restatement of the rules, the
scaler-driven AdamW against the plain one, the trainer in fp32 mode (where a power-of-two scale is exact) against the
unscaled trainer, the skip path, the fp16 storage mode on gradients that underflow without a scale, overflow inside the
f16 images, and two data-parallel ranks agreeing on a skipped step."""
import dataclasses
import os
import socket
import time
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

LR, BETAS, EPS, WD = 2e-4, (0.9, 0.999), 1e-8, 1e-2
ULP = 2.0 ** -23
ADAMW_TOL = 4 * LR * ULP  # one ulp on each of the two device-computed bias-correction floats; the rest is identical


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------ the rules, restated
def _rules(st, found, growth=2.0, backoff=0.5, interval=2000, lr=LR, betas=BETAS):
    """st: dict(scale, tracker, step, skipped) -> the record after clipfs_scaler_decide."""
    new = dict(st, found=0, inv_scale=np.float32(1.0) / np.float32(st["scale"]))
    if found:
        new.update(skipped=st["skipped"] + 1, skip=1, tracker=0, scale=np.float32(st["scale"]) * np.float32(backoff))
        return new
    new.update(step=st["step"] + 1, skip=0, tracker=st["tracker"] + 1)
    # lr and the betas cross the C ABI as fp32; the expressions are then evaluated in double, as clipfs_adamw does
    lr, b1, b2 = (float(np.float32(x)) for x in (lr, betas[0], betas[1]))
    new["inv_sqrt_bc2"] = np.float32(1.0 / np.sqrt(1.0 - b2 ** new["step"]))
    new["step_size"] = np.float32(lr / (1.0 - b1 ** new["step"]))
    if interval > 0 and new["tracker"] >= interval:
        new.update(scale=np.float32(st["scale"]) * np.float32(growth), tracker=0)
    return new


def _record(dev, scale, tracker=0, step=0, skipped=0):
    from clipfs import _lib, ops
    st = ops.new_scaler_state(scale, dev)
    si = st.view(torch.int32)
    si[_lib.SCALER_TRACKER], si[_lib.SCALER_STEP], si[_lib.SCALER_SKIPPED] = tracker, step, skipped
    return st


def _read(st):
    from clipfs import _lib as K
    f = st.cpu()
    i = f.view(torch.int32)
    return dict(scale=f[K.SCALER_SCALE].item(), inv_scale=f[K.SCALER_INV_SCALE].item(), found=i[K.SCALER_FOUND].item(),
                tracker=i[K.SCALER_TRACKER].item(), step=i[K.SCALER_STEP].item(), skipped=i[K.SCALER_SKIPPED].item(),
                inv_sqrt_bc2=f[K.SCALER_INV_SQRT_BC2].item(), step_size=f[K.SCALER_STEP_SIZE].item(),
                skip=i[K.SCALER_SKIP].item())


def _check_record(got, want):
    for k in ("scale", "inv_scale", "found", "tracker", "step", "skipped", "skip"):
        assert got[k] == want[k], (k, got, want)
    for k in ("inv_sqrt_bc2", "step_size"):  # double arithmetic on both sides, rounded to fp32: at most one ulp apart
        if k in want:
            assert abs(got[k] - float(want[k])) <= ULP * abs(float(want[k])), (k, got, want)


# ---------------------------------------------------------------------------- clipfs_grads_nonfinite + _scaler_decide
SIZES = [1, 3, 255, 256, 257, 1024 * 4 + 1, 8192 * 256 * 4 + 3]


@pytest.mark.parametrize("n", SIZES)
def test_nonfinite_check_and_decision(dev, n):
    from clipfs import _lib, ops
    # finite filler with the extremes that must NOT trip the check: fp32 maximum magnitude and subnormals
    gen = torch.Generator().manual_seed(n)
    special = torch.tensor([3.4e38, -3.4e38, 1e-40, -1e-40, 0.0, 1.0, -65504.0, 3.0e-8], dtype=torch.float32)
    host = special[torch.randint(0, len(special), (n + 1,), generator=gen)]
    mixed = torch.randn(n + 1, generator=gen)
    base = torch.where(torch.rand(n + 1, generator=gen) < 0.5, host, mixed).to(dev)
    nan, inf = float("nan"), float("inf")
    # (slice offset, index inside the slice or None, value): offset 1 is the base pointer that is not 16-byte aligned
    cases = [(0, None, 0.0), (0, 0, nan), (0, n - 1, nan), (0, n // 2, nan), (0, n // 2, inf), (0, n - 1, -inf),
             (0, 0, -inf), (1, None, 0.0), (1, 0, nan), (1, n - 1, nan), (1, n // 2, inf), (1, n // 3, -inf)]
    before = dict(scale=1024.0, tracker=1, step=4, skipped=2)
    for off, idx, val in cases:
        g = base[off:off + n]
        assert g.data_ptr() % 16 == 4 * off
        # the float just outside the slice is poison: reading past either end would trip the check
        outside = n if off == 0 else 0
        keep_out = base[outside].clone()
        base[outside] = nan
        if idx is not None:
            keep = g[idx].clone()
            g[idx] = val
        st = _record(dev, **before)
        ops.grads_nonfinite(g, st)
        flag = st.view(torch.int32)[_lib.SCALER_FOUND].item()
        ops.scaler_decide(st, LR, BETAS, 2.0, 0.5, 2)
        got = _read(st)
        if idx is not None:
            g[idx] = keep
        base[outside] = keep_out
        assert flag == (0 if idx is None else 1), (off, idx, val, flag)
        _check_record(got, _rules(before, flag, interval=2))


def test_decision_sequences(dev):
    """Growth after `interval` clean steps, backoff and tracker reset on a found step, a static scale that only skips."""
    from clipfs import _lib, ops
    for growth, backoff, interval, scale0 in ((2.0, 0.5, 3, 65536.0), (4.0, 0.25, 1, 8.0), (1.0, 1.0, 0, 1000.0)):
        st = _record(dev, scale0)
        want = dict(scale=scale0, tracker=0, step=0, skipped=0)
        for found in (0, 0, 1, 0, 0, 0, 0, 1, 1, 0):
            st.view(torch.int32)[_lib.SCALER_FOUND] = found
            ops.scaler_decide(st, LR, BETAS, growth, backoff, interval)
            want = _rules(want, found, growth, backoff, interval)
            _check_record(_read(st), want)
    # a scale at the top of fp32 does not grow into infinity
    st = _record(dev, 2.0 ** 127)
    ops.scaler_decide(st, LR, BETAS, 2.0, 0.5, 1)
    assert _read(st)["scale"] == 2.0 ** 127


# ------------------------------------------------------------------------------------------------ clipfs_adamw_scaled
def _adam_state(dev, n, steps, seed):
    """p, m, v after `steps` plain AdamW steps on random gradients (moments as training leaves them)."""
    from clipfs import ops
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen).to(dev)
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    for t in range(1, steps + 1):
        ops.adamw(p, torch.randn(n, generator=gen).to(dev), m, v, t, LR, BETAS, EPS, WD, 1.0)
    return p, m, v, torch.randn(n, generator=gen).to(dev)


@pytest.mark.parametrize("k", [0, 10, 40])
def test_adamw_scaled_clean_step_equals_plain_adamw(dev, k):
    from clipfs import ops
    n = 1003
    p, m, v, g = _adam_state(dev, n, 4, seed=7)
    scaled = g * 2.0 ** k  # exact
    want = [x.clone() for x in (p, m, v)]
    ops.adamw(want[0], scaled, want[1], want[2], 5, LR, BETAS, EPS, WD, 2.0 ** -k)
    st = _record(dev, 2.0 ** k, step=4)
    ops.grads_nonfinite(scaled, st)
    ops.scaler_decide(st, LR, BETAS, 2.0, 0.5, 2000)
    ops.adamw_scaled(p, scaled, m, v, st, LR, BETAS, EPS, WD)
    rec = _read(st)
    assert (rec["step"], rec["skip"], rec["skipped"], rec["tracker"]) == (5, 0, 0, 1)
    assert not torch.equal(p, _adam_state(dev, n, 4, seed=7)[0])  # the step was applied
    err = (p - want[0]).abs().max().item()
    print(f"adamw_scaled k={k}: max |p - plain| = {err:.3e} (bound {ADAMW_TOL:.3e})")
    assert err <= ADAMW_TOL
    # m and v never see the bias corrections: identical arithmetic
    assert torch.equal(m, want[1]) and torch.equal(v, want[2])


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_adamw_scaled_skipped_step_writes_nothing(dev, bad):
    from clipfs import ops
    n = 1003
    p, m, v, g = _adam_state(dev, n, 4, seed=9)
    g[n - 2] = bad
    keep = [x.clone() for x in (p, m, v)]
    st = _record(dev, 65536.0, tracker=7, step=4)
    ops.grads_nonfinite(g, st)
    ops.scaler_decide(st, LR, BETAS, 2.0, 0.5, 2000)
    ops.adamw_scaled(p, g, m, v, st, LR, BETAS, EPS, WD)
    rec = _read(st)
    assert (rec["step"], rec["skip"], rec["skipped"], rec["tracker"], rec["scale"]) == (4, 1, 1, 0, 32768.0)
    for got, want in zip((p, m, v), keep):  # bitwise: not even the weight decay ran
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_cross_entropy_scale_is_read_from_the_record(dev):
    """dlogits carry grad_scale * SCALE (exactly, for a power of two); loss sum and hit count are the unscaled ones."""
    from clipfs import ops
    gen = torch.Generator().manual_seed(3)
    logits = (torch.randn(7, 13, generator=gen) * 5).to(dev)
    tgt = torch.randint(0, 13, (7,), generator=gen).to(dev)
    loss, dl, hit = ops.cross_entropy(logits, tgt, True, grad_scale=0.5)
    st = _record(dev, 2.0 ** 20)
    loss_s, dl_s, hit_s = ops.cross_entropy(logits, tgt, True, grad_scale=0.5, scale_state=st)
    assert torch.equal(loss, loss_s) and torch.equal(hit, hit_s)
    assert torch.equal(dl_s, dl * 2.0 ** 20)


# --------------------------------------------------------------------------------------------------------- trainer
def _make(dev, cfg, backbone, r):
    """Model with rank-r q/k/v adapters in every block of both towers (synthetic adapter weights, B != 0)."""
    import lora_train_vlp as L
    from clipfs import synth
    from jclip.model import build_model
    sd = synth.synth_state_dict(cfg, seed=17, perturb=True)
    model = build_model(sd, device=dev)
    args = types.SimpleNamespace(encoder="both", position="all", backbone=backbone, params=["q", "k", "v"], r=r, alpha=1,
                                 dropout_rate=0.0)
    saved_t, saved_v = L.INDEX_POSITIONS_TEXT["all"], L.INDEX_POSITIONS_VISION.get(backbone)
    L.INDEX_POSITIONS_TEXT["all"] = list(range(cfg.transformer_layers))
    L.INDEX_POSITIONS_VISION[backbone] = {"all": list(range(cfg.vision_layers))}
    try:
        layers = L.apply_lora(args, model)
    finally:
        L.INDEX_POSITIONS_TEXT["all"] = saved_t
        if saved_v is None:
            del L.INDEX_POSITIONS_VISION[backbone]
        else:
            L.INDEX_POSITIONS_VISION[backbone] = saved_v
    lw = synth.synth_lora(cfg, r, seed=5)
    names = {"q": "q_proj", "k": "k_proj", "v": "v_proj"}
    with torch.no_grad():
        for i, layer in enumerate(layers):
            for pr in "qkv":
                mod = getattr(layer, names[pr])
                mod.w_lora_A.copy_(torch.from_numpy(lw[f"layer_{i}"][names[pr]]["w_lora_A"]))
                mod.w_lora_B.copy_(torch.from_numpy(lw[f"layer_{i}"][names[pr]]["w_lora_B"]))
    model.eval()
    return L, model


def _batch(dev, cfg, B=4, Cn=6, max_len=12):
    from clipfs import synth
    return (synth.synth_images(B, cfg.image_resolution, seed=3).to(dev),
            synth.synth_captions(Cn, cfg.context_length, cfg.vocab_size, seed=4, max_len=max_len).to(dev),
            synth.synth_labels(B, Cn, seed=2).to(dev))


def _tiny_trainer(dev, **kw):
    from clipfs import synth
    L, model = _make(dev, synth.TINY, "tiny", 4)
    return L.LoRATrainer(model, lr=LR, **kw)


@pytest.fixture(scope="module")
def tiny_unscaled(dev):
    """Three unscaled steps on TINY: the gradient of the first and the parameters after each (computed once)."""
    from clipfs import synth
    tr = _tiny_trainer(dev)
    img, cap, tgt = _batch(dev, synth.TINY)
    out = dict(params=[])
    for s in range(3):
        tr.flat.zero_grad()
        tr.forward_backward(img, cap, tgt)
        if s == 0:
            out["grad"] = tr.flat.grads.clone()
        tr.optimizer_step()
        out["params"].append(tr.flat.params.clone())
    out["m"], out["v"] = tr.flat.m.clone(), tr.flat.v.clone()
    assert tr.optimizer_steps == tr.t == 3 and tr.skipped_steps == 0 and tr.loss_scale_value is None
    return out


@pytest.mark.parametrize("mode", ["static", "dynamic"])
def test_fp32_scaled_steps_equal_unscaled_steps(dev, tiny_unscaled, mode):
    from clipfs import synth
    kw = dict(loss_scale=2.0 ** 12) if mode == "static" else dict(loss_scale="dynamic", init_scale=2.0 ** 12,
                                                                  growth_interval=2)
    tr = _tiny_trainer(dev, **kw)
    img, cap, tgt = _batch(dev, synth.TINY)
    want_g = tiny_unscaled["grad"]
    gmax = want_g.abs().max().item()
    assert gmax > 1e-5
    scales = [tr.loss_scale_value]
    for s in range(3):
        tr.flat.zero_grad()
        tr.forward_backward(img, cap, tgt)
        if s == 0:  # a power-of-two scale is exact in fp32: bitwise equality expected, the project's 1e-4 asserted
            g = tr.flat.grads * 2.0 ** -12
            err = (g - want_g).abs().max().item()
            print(f"{mode}: max |grad * 2^-12 - unscaled grad| = {err:.3e} of largest entry {gmax:.3e}")
            assert err <= 1e-4 * gmax
        tr.optimizer_step()
        scales.append(tr.loss_scale_value)
        err = (tr.flat.params - tiny_unscaled["params"][s]).abs().max().item()
        print(f"{mode}: step {s + 1}: max |param - unscaled| = {err:.3e} (bound {(s + 1) * ADAMW_TOL:.3e})")
        assert err <= (s + 1) * ADAMW_TOL
    assert (tr.flat.params - tiny_unscaled["params"][2]).abs().max().item() <= 3 * ADAMW_TOL
    assert not torch.equal(tr.flat.params, tiny_unscaled["params"][0])
    assert (tr.optimizer_steps, tr.skipped_steps, tr.t) == (3, 0, 3)
    if mode == "static":
        assert scales == [4096.0] * 4
    else:  # the scale doubles after the second clean step; the third step ran under 8192 and is still equivalent
        assert scales == [4096.0, 4096.0, 8192.0, 8192.0]


def test_skip_path(dev, tiny_unscaled):
    from clipfs import synth
    tr = _tiny_trainer(dev, loss_scale="dynamic")
    img, cap, tgt = _batch(dev, synth.TINY)
    assert tr.loss_scale_value == 65536.0
    tr.flat.zero_grad()
    tr.forward_backward(img, cap, tgt)
    keep = [x.clone() for x in (tr.flat.params, tr.flat.m, tr.flat.v)]
    tr.flat.grads[tr.flat.numel // 2] = float("inf")
    tr.optimizer_step()
    for got, want in zip((tr.flat.params, tr.flat.m, tr.flat.v), keep):
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert (tr.skipped_steps, tr.optimizer_steps, tr.t, tr.loss_scale_value) == (1, 0, 1, 32768.0)
    # the next clean step is AdamW's step 1 (bias correction of step 1), as a fresh trainer's first step
    tr.step(img, cap, tgt)
    assert (tr.skipped_steps, tr.optimizer_steps, tr.t, tr.loss_scale_value) == (1, 1, 2, 32768.0)
    err = (tr.flat.params - tiny_unscaled["params"][0]).abs().max().item()
    print(f"step after a skip vs a fresh first step: {err:.3e} (bound {ADAMW_TOL:.3e})")
    assert err <= ADAMW_TOL


def test_gradient_accumulation_under_one_scale(dev, tiny_unscaled):
    """Two forward_backward calls before one optimizer_step: the buffer holds twice the scaled gradient."""
    from clipfs import synth
    tr = _tiny_trainer(dev, loss_scale=2.0 ** 12)
    img, cap, tgt = _batch(dev, synth.TINY)
    tr.flat.zero_grad()
    tr.forward_backward(img, cap, tgt)
    tr.forward_backward(img, cap, tgt)
    want = tiny_unscaled["grad"] * 2.0 ** 13
    assert (tr.flat.grads - want).abs().max().item() <= 1e-4 * want.abs().max().item()


# ------------------------------------------------------------------------------------------ fp16 storage mode (L/14)
L14 = dict(r=16, B=4, Cn=6)


@pytest.fixture(scope="module")
def l14(dev):
    """ViT-L/14 shapes at depth 2 + 2 (the setup of test_fp16_precision_mode_l14) and its fp32 gradient, once."""
    from clipfs import synth
    cfg = dataclasses.replace(synth.VIT_L14, vision_layers=2, transformer_layers=2, vocab_size=2048)
    L, model = _make(dev, cfg, "ViT-L/14", L14["r"])
    batch = _batch(dev, cfg, L14["B"], L14["Cn"], max_len=20)
    model.engine.precision = "fp32"
    tr = L.LoRATrainer(model)
    tr.flat.zero_grad()
    tr.forward_backward(*batch, 1, L14["B"])
    ref = tr.flat.grads.clone()
    assert torch.isfinite(ref).all() and ref.abs().max().item() > 1e-5
    return L, model, batch, ref


def test_fp16_mode_underflow_without_and_with_loss_scale(dev, l14):
    """Logits gradients of 2^-40 of their usual size: below 1e-12, and every image-side gradient below about 1e-10, far
    under the 3e-8 at which f16 rounds to zero.  Unscaled (arm A) the f16 images are zeros and the gradient is lost;
    with loss_scale = 2^40 (arm B) the same call is within the fp16 budget of the fp32 gradient."""
    L, model, batch, ref = l14
    B = L14["B"]
    big = B * 2 ** 40
    rmax = ref.abs().max().item()
    model.engine.precision = "fp16"
    try:
        tr = L.LoRATrainer(model)
        tr.flat.zero_grad()
        tr.forward_backward(*batch, 1, big)
        a = tr.flat.grads * 2.0 ** 40
        err_a = (a - ref).abs().max().item()
        print(f"arm A (unscaled): max error {err_a:.3e} of largest reference entry {rmax:.3e} "
              f"({(a == 0).float().mean().item():.3f} of the entries exactly zero)")
        assert err_a > 0.5 * rmax  # the inputs really underflow
        tr = L.LoRATrainer(model, loss_scale=2.0 ** 40)
        tr.flat.zero_grad()
        tr.forward_backward(*batch, 1, big)
        b = tr.flat.grads  # (buffer / scale = the gradient at global_batch `big`) * 2^40 = the buffer itself
        err_b = (b - ref).abs().max().item()
        print(f"arm B (loss_scale 2^40): max error {err_b:.3e} of largest reference entry {rmax:.3e}")
        assert torch.isfinite(tr.flat.grads).all()
        assert err_b < 3e-2 * rmax
    finally:
        model.engine.precision = "fp32"


def test_fp16_mode_overflow_skips_the_step(dev, l14):
    """A scale of 2^60 overflows the f16 images: inf / NaN in the gradient are ordinary floating point, the step is
    skipped and the scale halved."""
    L, model, batch, ref = l14
    model.engine.precision = "fp16"
    try:
        tr = L.LoRATrainer(model, loss_scale="dynamic", init_scale=2.0 ** 60)
        keep = [x.clone() for x in (tr.flat.params, tr.flat.m, tr.flat.v)]
        tr.step(*batch, 1, L14["B"])
        assert not torch.isfinite(tr.flat.grads).all()
        for got, want in zip((tr.flat.params, tr.flat.m, tr.flat.v), keep):
            assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        assert (tr.skipped_steps, tr.optimizer_steps, tr.loss_scale_value) == (1, 0, 2.0 ** 59)
    finally:
        model.engine.precision = "fp32"


# --------------------------------------------------------------------------------------------------- data parallel
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_main(rank, world, port, out_dir):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for path in (os.path.join(root, "jittor-clip-fewshot_amd"), root):
        if path not in sys.path:
            sys.path.insert(0, path)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    from clipfs import dist as D
    from clipfs import synth
    dev = torch.device("cuda:0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    L, model = _make(dev, synth.TINY, "tiny", 4)
    img, cap, tgt = _batch(dev, synth.TINY)
    tr = L.LoRATrainer(model, lr=LR, loss_scale="dynamic")
    assert (tr.rank, tr.world) == (rank, world)
    lo, hi = D.shard_bounds(img.shape[0], rank, world)
    shard = (img[lo:hi].contiguous(), cap, tgt[lo:hi].contiguous(), 1, img.shape[0], lo)
    start = tr.flat.params.clone()
    tr.flat.zero_grad()
    tr.forward_backward(*shard)
    if rank == 1:  # only ONE rank's own gradient is bad: the all-reduce carries it to the other
        tr.flat.grads[3] = float("inf")
    tr.optimizer_step()
    after_skip = tr.flat.params.clone()
    rec1 = (tr.skipped_steps, tr.optimizer_steps, tr.loss_scale_value)
    tr.step(*shard)
    torch.cuda.synchronize()
    rec2 = (tr.skipped_steps, tr.optimizer_steps, tr.loss_scale_value)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), start=start.cpu().numpy(), after_skip=after_skip.cpu().numpy(),
             final=tr.flat.params.cpu().numpy(), rec1=np.array(rec1), rec2=np.array(rec2))
    dist.destroy_process_group()


def test_two_ranks_take_the_same_decision(tmp_path, dev):
    ctx = mp.spawn(_rank_main, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=False)
    deadline = time.monotonic() + 120  # each rank lives under this limit: a rank that hangs is killed, not waited for
    try:
        while not ctx.join(timeout=5):
            assert time.monotonic() < deadline, "a data-parallel rank did not finish in time"
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
    z = [np.load(os.path.join(str(tmp_path), f"rank{r}.npz")) for r in range(2)]
    for r in range(2):
        assert np.array_equal(z[r]["start"].view(np.int32), z[r]["after_skip"].view(np.int32))  # skipped on both ranks
        assert z[r]["rec1"].tolist() == [1, 0, 32768.0]
        assert z[r]["rec2"].tolist() == [1, 1, 32768.0]
        assert not np.array_equal(z[r]["final"], z[r]["start"])  # the clean step was applied
    assert np.array_equal(z[0]["start"].view(np.int32), z[1]["start"].view(np.int32))
    assert np.array_equal(z[0]["final"].view(np.int32), z[1]["final"].view(np.int32))
