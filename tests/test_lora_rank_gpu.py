"""LoRA ranks 17 ... 64 through the fused path: the matrix-core adapter kernels (rank groups of 16), the GEMMs' LoRA
epilogues, a train step against the fp64 oracle, the packed text backward, the other precision modes, the direct block
call, checkpoints and the refusals.  Tolerances are the ones the rank <= 16 tests state for the same products."""
import dataclasses
import math
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAMES = {"q": "q_proj", "k": "k_proj", "v": "v_proj", "o": "proj"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def _err(got, want):
    return (got.detach().double().cpu() - want.detach().double().cpu()).abs().max().item()


def _close(got, want, atol, what=""):
    err = _err(got, want)
    assert err <= atol, f"{what}: max abs err {err:.3e} > {atol:.1e}"


# ------------------------------------------------------------------ 1. adapter kernels vs fp64
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("rows,width,r,nseg,mask", [(45, 512, 17, 3, 7), (333, 768, 24, 3, 5), (1100, 1024, 32, 1, 1),
                                                     (333, 512, 48, 3, 7), (45, 768, 63, 3, 5), (1100, 512, 64, 3, 7),
                                                     (333, 1024, 64, 1, 1), (1100, 768, 64, 3, 5)])
def test_lora_kernels_high_rank(dev, p, rows, width, r, nseg, mask):
    from clipfs import _lib, ops
    from oracle import clip_oracle as O
    seed, sb, scale = 0x1234ABCD5, 7, 0.5
    x = _rand(rows, width, seed=1)
    A = _rand(nseg * r, width, seed=2, scale=width ** -0.5).requires_grad_()
    Bm = _rand(nseg * width, r, seed=3, scale=0.1).requires_grad_()
    xs = x.clone().requires_grad_()
    ts, parts = [], []
    for s in range(nseg):
        if not (mask >> s) & 1:
            ts.append(torch.zeros(rows, r, dtype=torch.float64))
            parts.append(torch.zeros(rows, width, dtype=torch.float64))
            continue
        m = torch.ones(rows, width, dtype=torch.float64)
        if p > 0:
            m = torch.from_numpy(O.dropout_keep_mask(seed, sb + s, rows, width, p)).double() / (1 - p)
        t = (xs * m) @ A[s * r:(s + 1) * r].t()
        ts.append(t)
        parts.append(scale * t @ Bm[s * width:(s + 1) * width].t())
    y = torch.cat(parts, dim=1)
    D = lambda t: t.detach().float().to(dev)
    sd = seed if p > 0 else 0
    kb = ops.lora_keep_bits(rows, width, dev) if p > 0 else None
    t_gpu = ops.lora_down(D(x), D(A), r, nseg, seg_mask=mask, p=p, seed=sd, stream_base=sb, keep_bits=kb)
    _close(t_gpu, torch.cat(ts, dim=1), 2e-5, "lora down")
    dy = _rand(rows, nseg * width, seed=4)
    y.backward(dy)
    dA = torch.zeros(nseg * r, width, device=dev)
    dB = torch.zeros(nseg * width, r, device=dev)
    dx = torch.zeros(rows, width, device=dev)
    dt = ops.lora_bwd(D(dy), D(x), t_gpu, D(A), D(Bm), dA, dB, dx=dx, scale=scale, p=p, seed=sd, stream_base=sb,
                      seg_mask=mask)
    _close(dA, A.grad, 2e-4, "lora dA")
    _close(dB, Bm.grad, 2e-4, "lora dB")
    _close(dx, xs.grad, 2e-4, "lora dx")
    # frozen adapter: no dA / dB, bitwise the same dt and dx
    dx_f = torch.zeros_like(dx)
    dt_f = ops.lora_bwd(D(dy), D(x), t_gpu, D(A), D(Bm), None, None, dx=dx_f, scale=scale, p=p, seed=sd, stream_base=sb,
                        seg_mask=mask)
    assert torch.equal(dt_f, dt) and torch.equal(dx_f, dx)
    if p > 0:
        assert _lib.load().clipfs_lora_keep_bits_ok(width, width, r, nseg) == 1
        bits = kb.cpu().numpy().view(np.uint16)
        for s in range(nseg):
            if not (mask >> s) & 1:
                continue
            keep = O.dropout_keep_mask(seed, sb + s, rows, width, p).reshape(rows, width // 4, 4)
            got = np.stack([(bits >> (4 * s + e)) & 1 for e in range(4)], axis=-1).astype(bool)
            assert np.array_equal(got, keep), f"keep bits of segment {s}"
        dA2, dB2, dx2 = torch.zeros_like(dA), torch.zeros_like(dB), torch.zeros_like(dx)
        ops.lora_bwd(D(dy), D(x), t_gpu, D(A), D(Bm), dA2, dB2, dx=dx2, scale=scale, p=p, seed=sd, stream_base=sb,
                     seg_mask=mask, keep_bits=kb)
        assert torch.equal(dA2, dA) and torch.equal(dB2, dB) and torch.equal(dx2, dx)
    # the f16 image of dy (fp16 storage mode): on an f16-exact dy the same bits; on the fp32 dy within f16 rounding
    dy16 = D(dy).half()
    outs = []
    for g in (dy16.float(), dy16):
        a_, b_, x_ = torch.zeros_like(dA), torch.zeros_like(dB), torch.zeros_like(dx)
        ops.lora_bwd(g, D(x), t_gpu, D(A), D(Bm), a_, b_, dx=x_, scale=scale, p=p, seed=sd, stream_base=sb, seg_mask=mask,
                     keep_bits=kb)
        outs.append((a_, b_, x_))
    for a_, b_ in zip(*outs):
        assert torch.equal(a_, b_)
    for got, want in zip(outs[1], (dA, dB, dx)):
        assert (got - want).abs().max().item() <= 2e-3 * want.abs().max().item() + 1e-6


# ------------------------------------------------------------------ 2. GEMM LoRA epilogues
@pytest.mark.parametrize("r", [17, 32, 64])
@pytest.mark.parametrize("M,N,K", [(300, 384, 128), (1000, 2304, 768)])
def test_gemm_lora_epilogue_fp32_bf16x3(dev, r, M, N, K):
    from clipfs import ops
    segw = N // 3
    a, w = _rand(M, K, seed=3), _rand(N, K, seed=4, scale=K ** -0.5)
    bias, res = _rand(N, seed=5), _rand(M, N, seed=6)
    t, lb = _rand(M, 3 * r, seed=7), _rand(N, r, seed=8, scale=r ** -0.5)
    D = lambda x: x.float().to(dev)
    want = a @ w.t() + bias + res
    for s in range(3):
        want[:, s * segw:(s + 1) * segw] += 0.5 * t[:, s * r:(s + 1) * r] @ lb[s * segw:(s + 1) * segw].t()
    kw = dict(bias=D(bias), residual=D(res), lora_t=D(t), lora_b=D(lb), lora_seg_width=segw, lora_scale=0.5)
    _close(ops.gemm_nt(D(a), D(w), **kw), want, 1e-4, f"fp32 gemm + lora r {r}")
    _close(ops.gemm_nt(D(a), D(w), b_planes=ops.split_bf16(D(w)), **kw), want, 1e-4, f"bf16x3 gemm + lora r {r}")


@pytest.mark.parametrize("r", [17, 32, 64])
@pytest.mark.parametrize("M,N,K,act", [(2056, 1024, 1024, 0), (1100, 512, 2048, 1), (16484, 2048, 128, 1),
                                       (8192, 4096, 192, 0), (20480, 1024, 1024, 2), (2048, 2560, 128, 0),
                                       (2048 + 40, 2560, 192, 1), (700, 384, 128, 0)])
def test_gemm_f16_lora_high_rank(dev, r, M, N, K, act):
    """the f16 x f16 kernels (every tile configuration these shapes reach, the phased 256 x 256 one included) against
    fp64 on the f16-rounded operands: the LoRA term runs ceil(r / 16) or ceil(r / 32) extra K-steps."""
    from clipfs import ops
    g = torch.Generator().manual_seed(M + N + K + r)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) * K ** -0.5
    bias = torch.randn(N, generator=g)
    segw = N // 2 if N % 256 == 0 else N
    nseg = N // segw
    t = torch.randn(M, nseg * r, generator=g)
    lb = torch.randn(N, r, generator=g) * 0.1
    aux_in = torch.randn(M, N, generator=g) if act == 2 else None
    a16, w16 = a.to(dev).half(), ops.to_f16(w.to(dev))
    ref = a16.double() @ w16.double().T + bias.double().to(dev)  # fp64 on the device (rocBLAS), f16-rounded operands
    t16 = t.half().double().to(dev).view(M, nseg, r)
    lb16 = (0.25 * lb).half().double().to(dev)
    for s in range(nseg):
        ref[:, s * segw:(s + 1) * segw] += t16[:, s] @ lb16[s * segw:(s + 1) * segw].T
    aux_out = torch.empty(M, N, device=dev) if act == 1 else None
    if act == 1:
        ref = ref * torch.sigmoid(1.702 * ref)
    elif act == 2:
        ai = aux_in.double().to(dev)
        sg = torch.sigmoid(1.702 * ai)
        ref = ref * (sg * (1 + 1.702 * ai * (1 - sg)))
    out = ops.gemm_nt(None, w.to(dev), bias=bias.to(dev), act=act, aux_out=aux_out,
                      aux_in=None if aux_in is None else aux_in.to(dev), b_planes=w16, a16=a16, lora_t=t.to(dev),
                      lora_b=lb.to(dev), lora_seg_width=segw, lora_scale=0.25)
    scale = ref.abs().max().item()
    assert _err(out, ref) <= 2e-5 * scale + 1e-5


# ------------------------------------------------------------------ engine helpers
# vision 256 / 4 heads, text 128 / 2 heads: widths the matrix-core adapter kernels cover (SMALL's 192 is not)
RANK_CFG = dict(name="rank", embed_dim=128, image_resolution=96, vision_layers=2, vision_width=256, vision_patch_size=32,
                context_length=24, vocab_size=1024, transformer_width=128, transformer_layers=3)


def _cfg(**kw):
    from clipfs import synth
    return synth.ClipConfig(**{**RANK_CFG, **kw})


def _args(backbone, params=("q", "k", "v"), r=32, p=0.0):
    return types.SimpleNamespace(encoder="both", position="all", backbone=backbone, params=list(params), r=r, alpha=1,
                                 dropout_rate=p)


def _build(cfg, dev, seed=11):
    from clipfs import synth
    from jclip.model import build_model
    sd = synth.synth_state_dict(cfg, seed=seed, perturb=True)
    return sd, build_model(sd, device=dev)


def _apply(model, cfg, args, lw, monkey):
    import lora_train_vlp as L
    monkey.setitem(L.INDEX_POSITIONS_TEXT, args.position, list(range(cfg.transformer_layers)))
    monkey.setitem(L.INDEX_POSITIONS_VISION.setdefault(args.backbone, {}), args.position, list(range(cfg.vision_layers)))
    layers = L.apply_lora(args, model)
    with torch.no_grad():
        for i, layer in enumerate(layers):
            for pr in args.params:
                m = getattr(layer, NAMES[pr])
                m.w_lora_A.copy_(torch.from_numpy(lw[f"layer_{i}"][NAMES[pr]]["w_lora_A"]))
                m.w_lora_B.copy_(torch.from_numpy(lw[f"layer_{i}"][NAMES[pr]]["w_lora_B"]))
    return layers


def _oracle_lora(lw, cfg, requires_grad=False):
    nt = cfg.transformer_layers
    conv = lambda d: {p: {k: torch.from_numpy(v).double().requires_grad_(requires_grad) for k, v in ab.items()}
                      for p, ab in d.items()}
    return ({b: conv(lw[f"layer_{b}"]) for b in range(nt)},
            {b: conv(lw[f"layer_{nt + b}"]) for b in range(cfg.vision_layers)})


# ------------------------------------------------------------------ 3. one train step vs fp64
@pytest.mark.parametrize("r", [32, 64])
@pytest.mark.parametrize("params,p,with_ctx", [(("q", "k", "v"), 0.25, True), (("q", "v", "o"), 0.0, False)])
def test_train_step_high_rank(dev, monkeypatch, r, params, p, with_ctx):
    import lora_train_vlp as L
    from clipfs import synth
    from clipfs.engine import _mix_seed
    from oracle import clip_oracle as O
    cfg = _cfg()
    sd, model = _build(cfg, dev)
    args = _args("rank", params=params, r=r, p=p)
    lw = synth.synth_lora(cfg, r, seed=5, params=params)
    layers = _apply(model, cfg, args, lw, monkeypatch)
    L.mark_only_lora_as_trainable(model)
    B, Cn = 6, 9
    img = synth.synth_images(B, cfg.image_resolution, seed=3)
    cap = synth.synth_captions(Cn, cfg.context_length, cfg.vocab_size, seed=4, max_len=12)
    tgt = synth.synth_labels(B, Cn, seed=2)
    ctx = torch.nn.Parameter(sd["token_embedding.weight"][[5, 6, 7, 8]].clone().to(dev)) if with_ctx else None
    model.train()
    tr = L.LoRATrainer(model, prompt_ctx=ctx)
    tr.flat.zero_grad()
    loss_sum, correct, logits = tr.forward_backward(img.to(dev), cap.to(dev), tgt.to(dev))
    seed = _mix_seed(model.engine.seed_base, model.engine.step)

    sd64 = {k: v.double() for k, v in sd.items()}
    tl, vl = _oracle_lora(lw, cfg, requires_grad=True)

    def drops(width, seq, n, layers_n, stream0):
        if p == 0:
            return None
        out = {}
        for l in range(layers_n):
            d = {}
            for s, pr in enumerate(("q", "k", "v", "o")):
                if pr in params:
                    keep = O.dropout_keep_mask(seed, stream0 + 4 * l + s, n * seq, width, p)
                    d[NAMES[pr]] = (torch.from_numpy(keep).double() / (1 - p)).reshape(n, seq, width).permute(1, 0, 2)
            out[l] = d
        return out

    td = drops(cfg.transformer_width, cfg.context_length, Cn, cfg.transformer_layers, 0)
    vd = drops(cfg.vision_width, cfg.vision_tokens, B, cfg.vision_layers, 1000)
    octx = ctx.detach().double().cpu().requires_grad_() if with_ctx else None
    loss, wl = O.train_step_loss(sd64, img.double(), cap, tgt, tl, vl, O.lora_scaling(1, r), text_drops=td, vis_drops=vd,
                                 ctx=octx, text_chunk=Cn)
    loss.backward()
    assert layers[0].scaling == pytest.approx(1 / math.sqrt(r))
    assert _err(logits, wl) < 1e-3
    assert abs(loss_sum.item() / B - loss.item()) < 1e-4
    assert correct.item() == int((wl.argmax(1) == tgt).sum())
    assert torch.equal(L.ops.topk(logits, 5).cpu().long(), O.jt_topk(wl.float(), 5))
    blks = list(tl.values()) + list(vl.values())
    gmax = max(t.grad.abs().max().item() for blk in blks for ab in blk.values() for t in ab.values())
    worst = 0.0
    for i, layer in enumerate(layers):
        pairs = dict((id(prm), g) for prm, g in layer.trainable_pairs())
        for pr in params:
            m = getattr(layer, NAMES[pr])
            for nm, prm in (("w_lora_A", m.w_lora_A), ("w_lora_B", m.w_lora_B)):
                worst = max(worst, _err(pairs[id(prm)], blks[i][NAMES[pr]][nm].grad))
    assert worst < 1e-4 * max(gmax, 1e-3), f"LoRA grad err {worst:.3e} vs scale {gmax:.3e}"
    if with_ctx:
        assert _err(ctx.grad_slot, octx.grad) < 1e-4 * max(octx.grad.abs().max().item(), 1e-3)
    p0 = tr.flat.params.detach().clone().double().cpu()
    g0 = tr.flat.grads.detach().clone().double().cpu()
    tr.optimizer_step()
    want, _, _ = O.jt_adamw_step(p0, g0, torch.zeros_like(p0), torch.zeros_like(p0), 1)
    assert _err(tr.flat.params, want) < 1e-6


# ------------------------------------------------------------------ 4. ViT-B/32 widths, full depth
def test_vit_b32_full_size_rank64(dev):
    import lora_train_vlp as L
    from clipfs import synth
    from oracle import clip_oracle as O
    cfg = synth.VIT_B32
    sd, model = _build(cfg, dev, seed=1234)
    args = _args("ViT-B/32", r=64, p=0.25)
    layers = L.apply_lora(args, model)
    lw = synth.synth_lora(cfg, 64, seed=5)
    with torch.no_grad():
        for i, layer in enumerate(layers):
            for pr in "qkv":
                m = getattr(layer, NAMES[pr])
                m.w_lora_A.copy_(torch.from_numpy(lw[f"layer_{i}"][NAMES[pr]]["w_lora_A"]))
                m.w_lora_B.copy_(torch.from_numpy(lw[f"layer_{i}"][NAMES[pr]]["w_lora_B"]))
    tl, vl = _oracle_lora(lw, cfg)
    B, Cn = 8, 16
    img = synth.synth_images(B, 224, seed=0)
    cap = synth.synth_captions(Cn, 77, cfg.vocab_size, seed=1)
    sd64 = {k: v.double() for k, v in sd.items()}
    s = O.lora_scaling(1, 64)
    model.eval()
    with torch.no_grad():
        fi = model.encode_image(img.to(dev))
        ft = model.encode_text(cap.to(dev))
        logits = L.ops.gemm_nt(L.ops.l2norm_fwd(fi), L.ops.l2norm_fwd(ft), alpha=100.0)
        wi = O.encode_image(sd64, img.double(), vl, s)
        wt = O.encode_text(sd64, cap, tl, s)
        wl = 100.0 * O.l2_normalize(wi) @ O.l2_normalize(wt).t()
        zl = 100.0 * O.l2_normalize(O.encode_image(sd64, img.double())) @ O.l2_normalize(O.encode_text(sd64, cap)).t()
    assert _err(logits, wl) < 1e-3, _err(logits, wl)
    assert _err(wl, zl) > 1e-2, "adapters must change the logits (test is vacuous otherwise)"
    assert torch.equal(L.ops.topk(logits, 5).cpu().long(), O.jt_topk(wl.float(), 5))


# ------------------------------------------------------------------ 5. packed text backward at r = 32 with dropout
def _captions(lens, vocab=49408, seq=77, seed=9):
    rng = np.random.RandomState(seed)
    out = np.zeros((len(lens), seq), dtype=np.int64)
    for c, n in enumerate(lens):
        out[c, 0] = vocab - 2
        out[c, 1:n - 1] = rng.randint(1, vocab - 2, size=n - 2)
        out[c, n - 1] = vocab - 1
    return torch.from_numpy(out)


def test_packed_text_backward_rank32(dev):
    """the live-row text backward at r = 32 with dropout (the keep bits exist above r = 16 now) against the all-rows
    backward: loss and logits bitwise, gradients within 1e-5 of each tensor's scale, the packed rerun bitwise"""
    import lora_train_vlp as L
    from clipfs import synth
    from jclip.model import build_model
    cfg = synth.VIT_B32
    model = build_model(synth.synth_state_dict(cfg, seed=1234), device=dev)
    args = _args("ViT-B/32", r=32, p=0.25)
    layers = L.apply_lora(args, model)
    lw = synth.synth_lora(cfg, 32, seed=5)
    with torch.no_grad():
        for i, layer in enumerate(layers):
            for pr in "qkv":
                m = getattr(layer, NAMES[pr])
                m.w_lora_A.copy_(torch.from_numpy(lw[f"layer_{i}"][NAMES[pr]]["w_lora_A"]))
                m.w_lora_B.copy_(torch.from_numpy(lw[f"layer_{i}"][NAMES[pr]]["w_lora_B"]))
    L.mark_only_lora_as_trainable(model)
    model.train()
    rng = np.random.RandomState(4)
    cap = _captions(list(rng.randint(8, 30, size=40))).to(dev)
    ctx = torch.nn.Parameter(model.token_embedding.weight.data[[5, 6, 7, 8]].clone())
    tr = L.LoRATrainer(model, prompt_ctx=ctx, shard_text=False)
    img = synth.synth_images(8, cfg.image_resolution, seed=0).to(dev)
    tgt = synth.synth_labels(8, cap.shape[0], seed=2).to(dev)
    eng = model.engine
    out = {}
    for pack, k in ((True, 0), (False, 0), (True, 1)):
        eng.pack_text_backward = pack
        eng.step = 3
        tr.flat.zero_grad()
        loss, _, logits = tr.forward_backward(img, cap, tgt)
        torch.cuda.synchronize()
        out[(pack, k)] = (loss.clone(), logits.clone(), tr.flat.grads.clone())
    ids, seq = eng._effective_ids(cap.contiguous())
    _, R = eng._pack_plan(ids)
    assert eng.txt.pack_mode(ids.shape[0], R, 1, seq, tr.last_plan["text"]) == 1, "the text backward must take the packed rows"
    (lp_, lg_p, gp), (ld_, lg_d, gd) = out[(True, 0)], out[(False, 0)]
    assert torch.equal(lp_, ld_) and torch.equal(lg_p, lg_d)
    scale_all = gd.abs().max().item()
    assert scale_all > 0
    base = tr.flat.grads.data_ptr()
    for layer in layers:
        for _, g in layer.trainable_pairs():  # the gradient slots are views of the flat buffer
            off, n = (g.data_ptr() - base) // 4, g.numel()
            assert 0 <= off and off + n <= gp.numel()
            vp, vd = gp[off:off + n], gd[off:off + n]
            err = (vp - vd).abs().max().item()
            assert err <= 1e-5 * max(vd.abs().max().item(), 1e-3 * scale_all), (err, vd.abs().max().item())
    assert torch.equal(out[(True, 1)][1], lg_p) and torch.equal(out[(True, 1)][2], gp)


# ------------------------------------------------------------------ 6. bf16x3 and fp16 storage at r = 32, ViT-L/14 widths
def test_precision_modes_rank32_l14(dev, monkeypatch):
    import lora_train_vlp as L
    from clipfs import synth
    from oracle import clip_oracle as O
    cfg = dataclasses.replace(synth.VIT_L14, vision_layers=2, transformer_layers=2, vocab_size=2048)
    sd, model = _build(cfg, dev, seed=17)
    args = _args("ViT-L/14", r=32, p=0.0)
    lw = synth.synth_lora(cfg, 32, seed=5)
    _apply(model, cfg, args, lw, monkeypatch)
    L.mark_only_lora_as_trainable(model)
    B, Cn = 3, 5
    img = synth.synth_images(B, 224, seed=3)
    cap = synth.synth_captions(Cn, 77, cfg.vocab_size, seed=4, max_len=20)
    tgt = synth.synth_labels(B, Cn, seed=2)
    sd64 = {k: v.double() for k, v in sd.items()}
    tl, vl = _oracle_lora(lw, cfg)
    with torch.no_grad():
        _, wl = O.train_step_loss(sd64, img.double(), cap, tgt, tl, vl, O.lora_scaling(1, 32), text_chunk=Cn)
    model.eval()
    tr = L.LoRATrainer(model)
    res = {}
    for mode in ("fp32", "bf16x3", "fp16", "fp16"):
        model.engine.precision = mode
        model.engine.step = 0
        tr.flat.zero_grad()
        _, _, logits = tr.forward_backward(img.to(dev), cap.to(dev), tgt.to(dev))
        torch.cuda.synchronize()
        run = (logits.double().cpu(), tr.flat.grads.double().cpu().clone())
        if mode in res:
            assert torch.equal(run[0], res[mode][0]) and torch.equal(run[1], res[mode][1]), "fp16 step not reproducible"
        res[mode] = run
    e32, eb, eh = (_err(res[m][0], wl) for m in ("fp32", "bf16x3", "fp16"))
    assert e32 < 1e-3 and eb < 1e-3 and eh < 5e-2, (e32, eb, eh)
    assert eh > e32  # the mode really switched
    assert int(res["fp16"][0].argmax(1).eq(wl.argmax(1)).sum()) == B
    g32 = res["fp32"][1]
    assert (res["bf16x3"][1] - g32).abs().max() < 3e-3 * g32.abs().max()
    assert (res["fp16"][1] - g32).abs().max() < 1e-1 * g32.abs().max()


# ------------------------------------------------------------------ 7. direct block call and checkpoints
def test_direct_block_call_rank48(dev):
    import lora_train_vlp as L
    from clipfs import synth
    from jclip.model import Transformer
    from oracle import clip_oracle as O
    cfg = synth.VIT_B32
    full = synth.synth_state_dict(cfg, seed=1234)
    pre = "visual.transformer.resblocks.0."
    sd = {k: v.to(dev) for k, v in full.items() if k.startswith(pre)}
    tower = Transformer(sd, "visual.transformer", 768, 1, 12, causal=False)
    mha = L.PlainMultiheadAttentionLoRA(tower.resblocks[0].attn, enable_lora=["q", "k", "v"], r=48, lora_alpha=1,
                                        dropout_rate=0.0)
    lw = synth.synth_lora(dataclasses.replace(cfg, transformer_layers=0, vision_layers=1), 48, seed=5)["layer_0"]
    with torch.no_grad():
        for pr in ("q_proj", "k_proj", "v_proj"):
            getattr(mha, pr).w_lora_A.copy_(torch.from_numpy(lw[pr]["w_lora_A"]))
            getattr(mha, pr).w_lora_B.copy_(torch.from_numpy(lw[pr]["w_lora_B"]))
    mha.eval()
    x = _rand(50, 2, 768, seed=3)
    xd = x.float().to(dev)
    with torch.no_grad():
        y, w = mha(xd, xd, xd, need_weights=False, attn_mask=None)
    assert w is None
    blk = {k: v.double() for k, v in O._block_params(full, "visual.transformer", 0).items()}
    lora = {pr: {k: torch.from_numpy(v).double() for k, v in ab.items()} for pr, ab in lw.items()}
    want = O.mha_forward(x.float().double(), blk, 12, None, lora, O.lora_scaling(1, 48))
    _close(y, want, 2e-5, "block call r 48")


def test_save_load_rank64(dev, monkeypatch, tmp_path):
    import lora_train_vlp as L
    from clipfs import synth
    cfg = _cfg()
    _, model = _build(cfg, dev)
    args = _args("rank", r=64)
    layers = _apply(model, cfg, args, synth.synth_lora(cfg, 64, seed=9), monkeypatch)
    path = str(tmp_path / "lora_weights1" / "lora_weights.pkl")
    L.save_lora(args, 0, layers, save_path=path)
    _, model2 = _build(cfg, dev)
    layers2 = _apply(model2, cfg, args, synth.synth_lora(cfg, 64, seed=10), monkeypatch)
    L.load_lora(args, layers2, path)
    for a, b in zip(layers, layers2):
        assert torch.equal(a.lora_A_qkv, b.lora_A_qkv) and torch.equal(a.lora_B_qkv, b.lora_B_qkv)
    _, model3 = _build(cfg, dev)
    args32 = _args("rank", r=32)
    layers3 = _apply(model3, cfg, args32, synth.synth_lora(cfg, 32, seed=10), monkeypatch)
    with pytest.raises(ValueError):
        L.load_lora(args32, layers3, path)


# ------------------------------------------------------------------ 8. refusals
@pytest.mark.parametrize("r,vision_width", [(65, 256), (32, 192)])
def test_refused_ranks(dev, monkeypatch, r, vision_width):
    import lora_train_vlp as L
    from clipfs import synth
    from clipfs._lib import ClipfsError
    cfg = _cfg(vision_width=vision_width)
    _, model = _build(cfg, dev)
    args = _args("rank", r=r)
    layers = _apply(model, cfg, args, synth.synth_lora(cfg, r, seed=5), monkeypatch)  # apply_lora accepts any rank
    before = [p.detach().clone() for layer in layers for p, _ in layer.trainable_pairs()]
    img = synth.synth_images(2, cfg.image_resolution, seed=3).to(dev)
    cap = synth.synth_captions(3, cfg.context_length, cfg.vocab_size, seed=4, max_len=12).to(dev)
    tgt = synth.synth_labels(2, 3, seed=2).to(dev)
    model.train()
    tr = L.LoRATrainer(model)
    with pytest.raises((ClipfsError, ValueError)) as ei:
        tr.step(img, cap, tgt)
    msg = str(ei.value)
    assert f"rank {r}" in msg and "width" in msg, msg
    after = [p.detach() for layer in layers for p, _ in layer.trainable_pairs()]
    assert all(torch.equal(a, b) for a, b in zip(before, after))
