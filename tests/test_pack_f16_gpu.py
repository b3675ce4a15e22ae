"""Packed (live-row) text backward of the fp16 storage mode: the f16 matrix-core attention backward on packed rows
(clipfs_attention_f16_bwd_packed), the row-mapped LayerNorm backward with an f16 image (clipfs_layernorm_bwd_rows_f16),
and full steps on ViT-L/14 shapes with Engine.pack_text_backward on and off.

Kernels: the packed results are BITWISE the dense kernels' on the live rows (given dO = 0 on the dead rows).
Steps: the forward is the same in both runs, so loss and logits are bitwise equal; the gradients of the packed and the
dense fp16 backward meet different GEMM tiles (R rows instead of M) and are held to the budget
test_fp16_precision_mode_l14 grants two fp16 paths, 1e-2 of the largest fp32-mode gradient, and to that test's
fp16-vs-fp32 budget, 3e-2 of it."""
import dataclasses
import functools
import itertools
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- 1. attention ------------------------------------------------------------------------------------------------------
B, H = 5, 8
ATT_CASES = [(77, 2), (77, 32), (77, 33), (77, 64), (77, 65), (77, 77), (41, 41), (33, 9), (32, 32), (96, 50)]


def _lens(seq, L):
    return torch.tensor([L, max(1, L // 2), 1, L, min(seq, L + 3)], dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def _att_inputs(seq, L):
    """f16-representable qkv and dO (zero on the dead rows), and the fp64 autograd gradient of the oracle's sdpa: computed
    once per (seq, L), shared by the four storage combinations and left unchanged."""
    from oracle import clip_oracle as O
    d = 64 * H
    lens = _lens(seq, L)
    g = torch.Generator().manual_seed(100 * seq + L)
    qkv = torch.randn(B * seq, 3 * d, generator=g).half().float()
    dout = torch.randn(B * seq, d, generator=g).half().float()
    live = (torch.arange(seq)[None, :] < lens[:, None]).reshape(-1)
    dout[~live] = 0
    mask = O.build_causal_mask(seq, torch.float64)
    q, k, v = (qkv.double().reshape(B, seq, 3, H, 64).permute(2, 0, 3, 1, 4)[i].clone().requires_grad_() for i in range(3))
    o = O.sdpa(q, k, v, mask)
    o.backward(dout.double().reshape(B, seq, H, 64).permute(0, 2, 1, 3))
    ref = torch.cat([t.grad.permute(0, 2, 1, 3).reshape(B * seq, d) for t in (q, k, v)], 1)
    off = torch.zeros(B + 1, dtype=torch.int32)
    off[1:] = torch.cumsum(lens, 0).to(torch.int32)
    return qkv, dout, live, ref, off


def _attention_pair(dev, seq, L, qkv_f16, dout_f16, want_fp32=True):
    """(packed fp32 | None, packed halves, dense fp32, dense halves, live, ref) for one case."""
    from clipfs import _lib, ops
    lib = _lib.load()
    d = 64 * H
    qkv, dout, live, ref, off = _att_inputs(seq, L)
    # the packed backward is the short backward of this length on the live rows, the dense records its forward's
    packed, dense = (_lib.attention_f16_plan(d, B, seq, H, True) for d in ("bwd_packed", "bwd"))
    assert packed == dense and packed["family"] == _lib.attention_f16_plan("fwd", B, seq, H, True)["family"] == "f16_short"
    qkv_d = qkv.to(dev)
    out, lse = ops.attention_f16_fwd(qkv_d, B, seq, H, True)  # the dense forward's records
    q_in = qkv_d.half() if qkv_f16 else qkv_d
    conv = (lambda t: t.half()) if dout_f16 else (lambda t: t)
    dout_full = conv(dout.to(dev)).contiguous()
    dout_p = conv(dout[live].contiguous().to(dev)).contiguous()
    R = int(off[-1])
    nan = float("nan")
    dq_p = torch.full((R, 3 * d), nan, device=dev) if want_fp32 else None
    dq16_p = torch.full((R, 3 * d), nan, device=dev, dtype=torch.float16)
    work_p = torch.full((B * H * seq,), nan, device=dev)
    off_d = off.to(dev)
    rc = lib.clipfs_attention_f16_bwd_packed(q_in.data_ptr(), int(qkv_f16), dout_p.data_ptr(), int(dout_f16), out.data_ptr(),
                                             lse.data_ptr(), None if dq_p is None else dq_p.data_ptr(), dq16_p.data_ptr(),
                                             work_p.data_ptr(), off_d.data_ptr(), B, seq, H, _stream())
    assert rc == 0, lib.clipfs_last_error()
    dq_f = torch.zeros(B * seq, 3 * d, device=dev)
    dq16_f = torch.zeros(B * seq, 3 * d, device=dev, dtype=torch.float16)
    work_f = torch.empty(B * H * seq, device=dev)
    rc = lib.clipfs_attention_f16_bwd(q_in.data_ptr(), int(qkv_f16), dout_full.data_ptr(), int(dout_f16), out.data_ptr(),
                                      lse.data_ptr(), dq_f.data_ptr(), dq16_f.data_ptr(), work_f.data_ptr(), B, seq, H, 1,
                                      _stream())
    assert rc == 0, lib.clipfs_last_error()
    torch.cuda.synchronize()
    return (None if dq_p is None else dq_p.cpu()), dq16_p.cpu(), dq_f.cpu(), dq16_f.cpu(), live, ref


@pytest.mark.parametrize("qkv_f16,dout_f16", list(itertools.product([0, 1], [0, 1])))
@pytest.mark.parametrize("seq,L", ATT_CASES)
def test_packed_attention(dev, seq, L, qkv_f16, dout_f16):
    """Captions of length L (and a mix: L // 2, 1, L + 3) in sequences of `seq` tokens, 1 ... 3 tiles of 32: bitwise the
    dense clipfs_attention_f16_bwd on the live rows, in the fp32 result and in the f16 image, and within the dense
    kernel's own budget of fp64 autograd (test_attention_f16_bwd: 1e-2 of the largest gradient entry, on f16-rounded
    inputs)."""
    got, got16, full, full16, live, ref = _attention_pair(dev, seq, L, qkv_f16, dout_f16)
    assert torch.isfinite(got).all() and torch.isfinite(got16.float()).all()
    assert torch.equal(got, full[live])
    assert torch.equal(got16, full16[live])
    want = ref[live]
    err = (got.double() - want).abs().max().item()
    print(f"seq {seq} L {L} qkv_f16 {qkv_f16} dout_f16 {dout_f16}: err {err:.3e} of max {want.abs().max().item():.3e}")
    assert err < 1e-2 * want.abs().max().item(), err


def test_packed_attention_f16_image_alone(dev):
    """dqkv == NULL (what the tower passes in fp16 storage mode): the f16 image is the dense kernel's."""
    got, got16, _, full16, live, _ = _attention_pair(dev, 77, 33, 1, 1, want_fp32=False)
    assert got is None
    assert torch.isfinite(got16.float()).all()
    assert torch.equal(got16, full16[live])


# ---- 2. LayerNorm ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["no_dres", "dres", "in_place"])
@pytest.mark.parametrize("rows", [37, 700])
def test_layernorm_bwd_rows_f16(dev, rows, mode):
    """clipfs_layernorm_bwd_rows_f16 against clipfs_layernorm_bwd_rows: the fp32 result bitwise, the f16 image bitwise
    its rounding; x / mean / rstd read through a random permutation subset of 1000 dense rows."""
    from clipfs import _lib
    lib = _lib.load()
    width, N = 768, 1000
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(N, width, generator=g).to(dev)
    gamma = (1 + 0.1 * torch.randn(width, generator=g)).to(dev)
    mean = x.mean(1).contiguous()
    rstd = (x.var(1, unbiased=False) + 1e-5).rsqrt().contiguous()
    xmap = torch.randperm(N, generator=g)[:rows].to(torch.int32).to(dev)
    dy = torch.randn(rows, width, generator=g).to(dev)
    res = torch.randn(rows, width, generator=g).to(dev)

    def run(f16):
        dres = None if mode == "no_dres" else res.clone()
        dx = dres if mode == "in_place" else torch.full((rows, width), float("nan"), device=dev)
        dx16 = torch.full((rows, width), float("nan"), device=dev, dtype=torch.float16)
        pr = None if dres is None else dres.data_ptr()
        if f16:
            rc = lib.clipfs_layernorm_bwd_rows_f16(dy.data_ptr(), x.data_ptr(), width, gamma.data_ptr(), mean.data_ptr(),
                                                   rstd.data_ptr(), xmap.data_ptr(), pr, dx.data_ptr(), dx16.data_ptr(), width,
                                                   rows, width, _stream())
        else:
            rc = lib.clipfs_layernorm_bwd_rows(dy.data_ptr(), x.data_ptr(), width, gamma.data_ptr(), mean.data_ptr(),
                                               rstd.data_ptr(), xmap.data_ptr(), pr, dx.data_ptr(), width, rows, width,
                                               _stream())
        assert rc == 0, lib.clipfs_last_error()
        torch.cuda.synchronize()
        return dx.cpu(), dx16.cpu()

    want, _ = run(False)
    got, got16 = run(True)
    assert torch.isfinite(want).all()
    assert torch.equal(got, want)
    assert torch.equal(got16, want.half())


# ---- 3 - 5. steps ------------------------------------------------------------------------------------------------------
NAMES = {"q": "q_proj", "k": "k_proj", "v": "v_proj"}
LENS_SHORT = [77, 2, 32, 33, 64, 65] + [int(x) for x in np.random.RandomState(3).randint(2, 20, size=34)]
LENS_LONG = [int(x) for x in np.random.RandomState(4).randint(50, 78, size=40)]


def _captions(lens, vocab, seq=77, seed=9):
    """ids [n, seq] with caption c's EOT at position lens[c] - 1 (lens[c] >= 2: SOT ... EOT)."""
    rng = np.random.RandomState(seed)
    out = np.zeros((len(lens), seq), dtype=np.int64)
    for c, n in enumerate(lens):
        out[c, 0] = vocab - 2
        out[c, 1:n - 1] = rng.randint(1, vocab - 2, size=n - 2)
        out[c, n - 1] = vocab - 1
    return torch.from_numpy(out)


class _Setup:
    """ViT-L/14 shapes at depth 2 + 2 (the model of test_fp16_precision_mode_l14), LoRA r = 16 on q / k / v with dropout
    0.25, 32 images, train mode."""

    def __init__(self, dev, with_ctx):
        import lora_train_vlp as L
        from clipfs import synth
        from jclip.model import build_model
        cfg = dataclasses.replace(synth.VIT_L14, vision_layers=2, transformer_layers=2, vocab_size=2048)
        sd = synth.synth_state_dict(cfg, seed=17, perturb=True)
        model = build_model(sd, design_details=None, device=dev)
        args = types.SimpleNamespace(encoder="both", position="all", backbone="ViT-L/14", params=["q", "k", "v"], r=16,
                                     alpha=1, dropout_rate=0.25)
        lw = synth.synth_lora(cfg, 16, seed=5)
        # apply_lora on a synthetic-depth model: the position tables cut to the model's depth for the call
        old_t = L.INDEX_POSITIONS_TEXT["all"]
        vis = L.INDEX_POSITIONS_VISION.setdefault("ViT-L/14", {})
        old_v = vis.get("all")
        L.INDEX_POSITIONS_TEXT["all"] = list(range(cfg.transformer_layers))
        vis["all"] = list(range(cfg.vision_layers))
        try:
            layers = L.apply_lora(args, model)
        finally:
            L.INDEX_POSITIONS_TEXT["all"] = old_t
            if old_v is None:
                del vis["all"]
            else:
                vis["all"] = old_v
        with torch.no_grad():
            for i, layer in enumerate(layers):
                for p in "qkv":
                    ab = lw[f"layer_{i}"][NAMES[p]]
                    m = getattr(layer, NAMES[p])
                    m.w_lora_A.copy_(torch.from_numpy(ab["w_lora_A"]))
                    m.w_lora_B.copy_(torch.from_numpy(ab["w_lora_B"]))
        model.train()
        ctx = torch.nn.Parameter(model.token_embedding.weight.data[[5, 6, 7, 8]].clone()) if with_ctx else None
        self.L, self.dev, self.cfg, self.model, self.layers = L, dev, cfg, model, layers
        self.tr = L.LoRATrainer(model, prompt_ctx=ctx, shard_text=False)
        self.img = synth.synth_images(32, 224, seed=3).to(dev)
        self.frozen = None  # the text block whose adapters are frozen (its gradient views hold a sentinel during a step)

    def step(self, cap, precision, pack):
        """(loss, logits, flat gradients) of one forward_backward with a fixed dropout seed."""
        from clipfs import synth
        eng = self.model.engine
        eng.precision = precision
        eng.trim_text = False
        eng.pack_text_backward = pack
        eng.step = 3
        tgt = synth.synth_labels(32, cap.shape[0], seed=2).to(self.dev)
        self.tr.flat.zero_grad()
        if self.frozen is not None:
            for _, g in self.frozen.trainable_pairs():
                g.fill_(7.0)
        loss, _, logits = self.tr.forward_backward(self.img, cap.to(self.dev), tgt)
        torch.cuda.synchronize()
        if self.frozen is not None:  # untouched: the sentinel is still there
            for _, g in self.frozen.trainable_pairs():
                assert torch.equal(g, torch.full_like(g, 7.0))
                g.zero_()
        return loss.clone(), logits.clone(), self.tr.flat.grads.clone()

    def packs(self, cap):
        """The library's decision for the fp16 text backward of this caption table."""
        eng = self.model.engine
        eng.precision = "fp16"
        eng.trim_text = False
        ids, seq = eng._effective_ids(cap.to(self.dev).contiguous())
        _, R = eng._pack_plan(ids)
        return eng.txt.pack_mode(ids.shape[0], R, 1, seq, self.tr.last_plan["text"]), R, ids.shape[0] * seq


@pytest.fixture(scope="module")
def l14(dev):
    return _Setup(dev, with_ctx=True)


def _check_step(s, cap, label):
    _, _, g32 = s.step(cap, "fp32", True)
    runs = [s.step(cap, "fp16", pack) for pack in (True, False, True)]
    mode, R, M = s.packs(cap)
    assert mode == 1 and 2 * R <= M and M >= 2048, (mode, R, M)
    for loss, logits, g in runs:
        assert torch.equal(loss, runs[0][0]) and torch.equal(logits, runs[0][1])
        assert torch.isfinite(g).all() and g.abs().max().item() > 0
    gp, gd = runs[0][2], runs[1][2]
    scale = g32.abs().max().item()
    assert scale > 0
    r_dense = (gp - gd).abs().max().item() / scale
    r_fp32 = (gp - g32).abs().max().item() / scale
    print(f"{label}: R {R} of M {M}; max|g_packed - g_dense| / max|g32| = {r_dense:.3e}; "
          f"max|g_packed - g32| / max|g32| = {r_fp32:.3e}; max|g_dense - g32| / max|g32| = "
          f"{(gd - g32).abs().max().item() / scale:.3e}")
    assert r_dense <= 1e-2, r_dense
    assert r_fp32 <= 3e-2, r_fp32
    assert torch.equal(runs[2][2], gp)  # two packed runs


def test_step_packed_vs_dense_vs_fp32(l14):
    """40 captions (EOT at 77, 2, 32, 33, 64, 65 and 34 short ones: 3 080 dense rows, R far below M / 2), prompt ctx.
    R = 601 live rows.  Measured on an MI355X: max|g_packed - g_dense| = 4.5e-9 and max|g_packed - g32| = 1.26e-3 of
    max|g32| (the dense fp16 backward is at the same 1.26e-3 of fp32)."""
    cap = _captions(LENS_SHORT, l14.cfg.vocab_size)
    _check_step(l14, cap, "step")
    assert l14.tr.last_plan["text"] == 0


def test_fallback_more_than_half_the_rows(l14):
    """R > M / 2: the switch changes nothing, the dense rows run either way."""
    cap = _captions(LENS_LONG, l14.cfg.vocab_size)
    on = l14.step(cap, "fp16", True)
    off = l14.step(cap, "fp16", False)
    mode, R, M = l14.packs(cap)
    assert mode == 0 and 2 * R > M
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1]) and torch.equal(on[2], off[2])
    assert on[2].abs().max().item() > 0


def test_gradient_floor(dev):
    """No prompt ctx and the lowest text block's adapters frozen: the walk stops above block 0 (grad_lo 1), whose slice
    of the flat gradient stays untouched.
    Measured on an MI355X: max|g_packed - g_dense| = 2.6e-7 and max|g_packed - g32| = 1.21e-3 of max|g32|."""
    s = _Setup(dev, with_ctx=False)
    s.frozen = s.layers[0]
    for prm, _ in s.frozen.trainable_pairs():
        prm.requires_grad_(False)
    cap = _captions(LENS_SHORT, s.cfg.vocab_size)
    _check_step(s, cap, "floor")
    assert s.tr.last_plan["text"] == 1
