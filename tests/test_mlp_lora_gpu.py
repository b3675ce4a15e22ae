"""LoRA adapters on the MLP linears (``params`` tokens ``c_fc`` / ``c_proj``) on the GPU: the rectangular adapter products,
the GEMM epilogues at the MLP shapes and the in-place QuickGELU' kernel against fp64 restatements, then whole trainer steps
against fp64 autograd on the CPU oracle.

The oracle has no MLP adapters.  ``_resblock`` below is its ``resblock_forward`` with LinearLoRA.execute
(``oracle.lora_linear``) on both MLP linears, installed over it with monkeypatch for the duration of a test; the dropout
masks are ``oracle.dropout_keep_mask`` at the streams stream0 + 500 + 2 l (c_fc) and + 1 (c_proj).  Every test gives the B
matrices random non-zero values: with B = 0, the initial state, the adapter path is invisible and dA is zero.

Bounds are those of the existing tests for the same quantities: t 2e-5 and dA / dB / dx 2e-4 absolute on O(1) data
(test_kernels_gpu.test_lora_down_and_bwd); GEMM epilogues 1e-4 (exact fp32) and 6e-5 (bf16x3) absolute on O(1) data
(test_gemm_epilogues, test_gemm_bf16x3); training logits 1e-3, loss 1e-4, adapter gradients 1e-4 of the largest gradient
entry (test_engine_gpu); bias gradients 1e-4 of the largest entry (test_bias_training_gpu); the three-step trajectory 2e-4
(test_three_step_training_trajectory); two ranks against one process 2e-5 of the largest gradient entry (test_dp_gpu)."""
import os
import socket
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

ATTN = {"q": "q_proj", "k": "k_proj", "v": "v_proj", "o": "proj"}
MLP = ("c_fc", "c_proj")
ALL6 = ("q", "k", "v", "o", "c_fc", "c_proj")


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


def _close(got, want, atol, what):
    err = _err(got, want)
    print(f"{what}: max abs err {err:.3e} (bound {atol:.1e})")
    assert err <= atol, f"{what}: max abs err {err:.3e} > {atol:.1e}"


def _gelu64(u):
    return u * torch.sigmoid(1.702 * u)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the adapter products, rectangular
# ---------------------------------------------------------------------------------------------------------------------

def _product_cases():
    out = []
    for fin, fout in ((128, 512), (512, 128), (64, 256), (256, 64), (192, 768), (768, 192)):
        for r in (4, 16) + ((17, 64) if fin % 128 == 0 else ()):
            for p in (0.0, 0.25):
                # the QuickGELU-on-load switch alternates over the grid, so both kernel families see it on and off
                out.append((300, fin, fout, r, p, (len(out) % 2) == 1))
    out.append((130, 3072, 768, 16, 0.25, True))
    out.append((130, 4096, 1024, 4, 0.0, True))
    out.append((130, 4096, 1024, 64, 0.25, False))
    return out


@pytest.mark.parametrize("rows,fin,fout,r,p,x_act", _product_cases())
def test_rectangular_products_against_fp64(dev, rows, fin, fout, r, p, x_act):
    """clipfs_lora_down and clipfs_lora_bwd_xact with an output width that differs from the input width: t, dt, dA, dB
    and dx accumulated into a non-zero tensor.  300 rows are ragged against every slice length (8 ... 2048).  Widths that
    are multiples of 128 run the matrix-core kernels, 64 and 192 the one-wave-per-row kernels.  dt is a row reduction
    of O(1) data like t and takes its bound."""
    from clipfs import ops
    from oracle import clip_oracle as O
    seed, sb, row0, scale = 0x1234ABCD5, 503, 40, 0.5
    u = _rand(rows, fin, seed=1).requires_grad_()
    A = _rand(r, fin, seed=2, scale=fin ** -0.5).requires_grad_()
    Bm = _rand(fout, r, seed=3, scale=0.1).requires_grad_()
    dy = _rand(rows, fout, seed=4)
    dx0 = _rand(rows, fin, seed=5)
    x = _gelu64(u) if x_act else u
    x.retain_grad()
    m = torch.ones(rows, fin, dtype=torch.float64)
    if p > 0:
        keep = O.dropout_keep_mask(seed, sb, row0 + rows, fin, p)[row0:]
        m = torch.from_numpy(keep).double() / (1 - p)
    t = (x * m) @ A.t()
    t.retain_grad()
    (scale * t @ Bm.t()).backward(dy)
    D = lambda v: v.detach().float().to(dev).contiguous()
    sd = seed if p > 0 else 0
    # forward: the down-projection reads the adapter's input itself (the forward has g = QuickGELU(u) in scratch)
    t_gpu = ops.lora_down(D(x), D(A), r, 1, p=p, seed=sd, stream_base=sb, row0=row0)
    _close(t_gpu, t, 2e-5, "t")

    def run(frozen):
        dA = None if frozen else torch.zeros(r, fin, device=dev)
        dB = None if frozen else torch.zeros(fout, r, device=dev)
        dx = D(dx0)
        dt = ops.lora_bwd_rect(D(dy), D(u) if x_act else D(x), t_gpu, D(A), D(Bm), dA, dB, dx=dx, scale=scale, p=p, seed=sd,
                               stream_base=sb, row0=row0, x_act=x_act)
        return dt, dA, dB, dx

    dt, dA, dB, dx = run(False)
    _close(dt, t.grad, 2e-5, "dt")
    _close(dA, A.grad, 2e-4, "dA")
    _close(dB, Bm.grad, 2e-4, "dB")
    _close(dx, dx0 + x.grad, 2e-4, "dx")  # with the switch: the gradient wrt QuickGELU(u)
    assert A.grad.abs().max().item() > 1e-2 and x.grad.abs().max().item() > 1e-3
    # two identical calls: bitwise
    dt2, dA2, dB2, dx2 = run(False)
    assert torch.equal(dt2, dt) and torch.equal(dA2, dA) and torch.equal(dB2, dB) and torch.equal(dx2, dx)
    # frozen adapter (no slots): dt and dx bitwise those of the call with slots
    dt3, _, _, dx3 = run(True)
    assert torch.equal(dt3, dt) and torch.equal(dx3, dx)


def test_square_calls_are_unchanged_by_the_new_entry_point(dev):
    """clipfs_lora_bwd_xact with x_act = 0 at a square shape is clipfs_lora_bwd, bit for bit."""
    from clipfs import ops
    rows, d, r = 300, 256, 8
    D = lambda v: v.float().to(dev).contiguous()
    x, A, Bm, dy = D(_rand(rows, d, seed=1)), D(_rand(r, d, seed=2, scale=d ** -0.5)), D(_rand(d, r, seed=3, scale=0.1)), D(_rand(rows, d, seed=4))
    t = ops.lora_down(x, A, r, 1, p=0.25, seed=9, stream_base=3)
    outs = []
    for fn in (ops.lora_bwd, ops.lora_bwd_rect):
        dA, dB, dx = torch.zeros(r, d, device=dev), torch.zeros(d, r, device=dev), torch.zeros(rows, d, device=dev)
        dt = fn(dy, x, t, A, Bm, dA, dB, dx=dx, scale=0.5, p=0.25, seed=9, stream_base=3)
        outs.append((dt, dA, dB, dx))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# 2. GEMM epilogues at the MLP shapes
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
@pytest.mark.parametrize("r", [4, 17])
def test_gemm_epilogues_at_mlp_shapes(dev, mode, r):
    """c_fc: (N, K) = (512, 128) with the rank-r up-projection (one segment of N columns), bias, QuickGELU and the saved
    pre-activation -- the adapter's term is inside the pre-activation.  c_proj: (128, 512) with the up-projection, bias
    and the residual.  B's entries are scaled by r^-1/2 so that the data stays O(1), which the absolute bounds assume."""
    from clipfs import ops
    M, bound = 300, {"fp32": 1e-4, "bf16x3": 6e-5}[mode]
    D = lambda v: v.float().to(dev).contiguous()
    for (N, K), gelu in (((512, 128), True), ((128, 512), False)):
        a, w = _rand(M, K, seed=3), _rand(N, K, seed=4, scale=K ** -0.5)
        bias, res = _rand(N, seed=5), _rand(M, N, seed=6)
        t, lb = _rand(M, r, seed=7), _rand(N, r, seed=8, scale=r ** -0.5)
        kw = dict(bias=D(bias), lora_t=D(t), lora_b=D(lb), lora_seg_width=N, lora_scale=0.5)
        if mode == "bf16x3":
            kw["b_planes"] = ops.split_bf16(D(w))
        pre = a @ w.t() + bias + 0.5 * t @ lb.t()
        assert (0.5 * t @ lb.t()).abs().max().item() > 0.5
        if gelu:
            u = torch.empty(M, N, device=dev)
            out = ops.gemm_nt(D(a), D(w), act=1, aux_out=u, **kw)
            _close(u, pre, bound, f"{mode} r={r} c_fc pre-activation")
            _close(out, _gelu64(pre), bound, f"{mode} r={r} c_fc QuickGELU")
        else:
            out = ops.gemm_nt(D(a), D(w), residual=D(res), **kw)
            _close(out, pre + res, bound, f"{mode} r={r} c_proj residual")


# ---------------------------------------------------------------------------------------------------------------------
# 3. dg *= QuickGELU'(u), in place
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(300, 512), (7, 129), (1, 3), (2307, 1024)])
def test_gelu_bwd_inplace(dev, shape):
    """Against fp64 autograd; 7 x 129 = 903 and 1 x 3 are no multiple of 4 (nor of 4 rows x 256 columns), 2307 x 1024 is
    more float4s than one pass of the grid covers.  fp32 rounding of an O(1) product: 1e-5."""
    from clipfs import ops
    u = _rand(*shape, seed=1, scale=2.0).requires_grad_()
    dg = _rand(*shape, seed=2)
    _gelu64(u).backward(dg)
    got = ops.gelu_bwd_inplace(dg.float().to(dev).contiguous(), u.detach().float().to(dev).contiguous())
    _close(got, u.grad, 1e-5, f"gelu' {shape}")


def test_unfused_gelu_bwd_equals_the_dgrad_epilogue(dev):
    """A block with a c_proj adapter runs the c_proj dgrad without act = 2 and applies QuickGELU' afterwards: with nothing
    added in between that is the fused epilogue's result, bit for bit (same fp32 product, same factor)."""
    from clipfs import ops
    M, N, K = 300, 512, 128
    D = lambda v: v.float().to(dev).contiguous()
    a, w, u = D(_rand(M, K, seed=1)), D(_rand(N, K, seed=2, scale=K ** -0.5)), D(_rand(M, N, seed=3, scale=2.0))
    fused = ops.gemm_nt(a, w, act=2, aux_in=u)
    assert torch.equal(ops.gelu_bwd_inplace(ops.gemm_nt(a, w), u), fused)


# ---------------------------------------------------------------------------------------------------------------------
# the fp64 block with MLP adapters, and a model + oracle pair
# ---------------------------------------------------------------------------------------------------------------------

def _resblock(x, blk, heads, attn_mask, lora=None, scaling=0.0, drop=None):
    """oracle.resblock_forward with LinearLoRA.execute on mlp.c_fc / mlp.c_proj (keys ``c_fc`` / ``c_proj`` of the block's
    adapter and dropout-multiplier dictionaries)."""
    from oracle import clip_oracle as O
    lora, drop = lora or {}, drop or {}
    h = O.jt_layer_norm(x, blk["ln_1.weight"], blk["ln_1.bias"])
    x = x + O.mha_forward(h, blk, heads, attn_mask, lora, scaling, drop or None)
    h = O.jt_layer_norm(x, blk["ln_2.weight"], blk["ln_2.bias"])
    fc, pr = lora.get("c_fc"), lora.get("c_proj")
    u = O.lora_linear(h, blk["mlp.c_fc.weight"], blk["mlp.c_fc.bias"], fc and fc["w_lora_A"], fc and fc["w_lora_B"], scaling,
                      drop.get("c_fc"))
    g = O.quick_gelu(u)
    y = O.lora_linear(g, blk["mlp.c_proj.weight"], blk["mlp.c_proj.bias"], pr and pr["w_lora_A"], pr and pr["w_lora_B"],
                      scaling, drop.get("c_proj"))
    return x + y


def _oname(tok):
    return ATTN.get(tok, tok)


def _make(dev, cfg_name, params, p=0.0, r=4, n_vpt=0, with_ctx=False, encoder="both", text_blocks=None, vision_blocks=None,
          bias="none"):
    """Model with adapters on ``params`` (every A and B random, B non-zero), trainable flags set, on ``dev``."""
    import lora_train_vlp as L
    from clipfs import synth
    from jclip.model import build_model
    cfg = getattr(synth, cfg_name)
    sd = synth.synth_state_dict(cfg, seed=11, perturb=True)
    model = build_model(sd, design_details={"vision_ctx": n_vpt} if n_vpt else None, device=dev)
    args = types.SimpleNamespace(encoder=encoder, position="all", backbone="synthetic", params=list(params), r=r, alpha=1,
                                 dropout_rate=p)
    tb = list(range(cfg.transformer_layers)) if text_blocks is None else list(text_blocks)
    vb = list(range(cfg.vision_layers)) if vision_blocks is None else list(vision_blocks)
    saved = L.INDEX_POSITIONS_TEXT["all"]
    L.INDEX_POSITIONS_TEXT["all"] = tb
    L.INDEX_POSITIONS_VISION["synthetic"] = {"all": vb}
    try:
        layers = L.apply_lora(args, model)
    finally:
        L.INDEX_POSITIONS_TEXT["all"] = saved
        del L.INDEX_POSITIONS_VISION["synthetic"]
    rng = np.random.RandomState(5)
    weights = []  # per list entry: {oracle name: {w_lora_A, w_lora_B}} as numpy
    with torch.no_grad():
        for layer in layers:
            w = {}
            for tok in params:
                m = getattr(layer, _oname(tok))
                fout, fin = m.w_lora_B.shape[0], m.w_lora_A.shape[1]
                a = rng.uniform(-1, 1, size=(r, fin)).astype(np.float32) / np.float32(np.sqrt(fin))
                b = (rng.standard_normal((fout, r)) * 0.05).astype(np.float32)
                m.w_lora_A.copy_(torch.from_numpy(a))
                m.w_lora_B.copy_(torch.from_numpy(b))
                w[_oname(tok)] = {"w_lora_A": a, "w_lora_B": b}
            weights.append(w)
    L.mark_only_lora_as_trainable(model, bias)
    if n_vpt:
        model.visual.VPT.requires_grad_(True)
    ctx = torch.nn.Parameter(sd["token_embedding.weight"][[5, 6, 7, 8]].clone().to(dev)) if with_ctx else None
    nt = len(tb) if encoder in ("text", "both") else 0
    return types.SimpleNamespace(L=L, cfg=cfg, sd=sd, model=model, layers=layers, weights=weights, params=tuple(params), p=p,
                                 r=r, ctx=ctx, n_vpt=n_vpt, text_blocks=tb[:nt] if nt else [],
                                 vision_blocks=vb if encoder in ("vision", "both") else [], dev=dev)


def _batch(cfg, B=6, Cn=9):
    from clipfs import synth
    return (synth.synth_images(B, cfg.image_resolution, seed=3),
            synth.synth_captions(Cn, cfg.context_length, cfg.vocab_size, seed=4, max_len=12),
            synth.synth_labels(B, Cn, seed=2))


def _oracle_state(S, bias_names=()):
    """fp64 leaves of the oracle: (sd64, text adapters {block: {...}}, vision adapters, vpt, ctx)."""
    sd64 = {k: v.double() for k, v in S.sd.items()}
    for n in bias_names:
        sd64[n].requires_grad_(True)
    conv = lambda w: {k: {n: torch.from_numpy(v).double().requires_grad_(True) for n, v in ab.items()} for k, ab in w.items()}
    nt = len(S.text_blocks)
    tl = {b: conv(S.weights[i]) for i, b in enumerate(S.text_blocks)}
    vl = {b: conv(S.weights[nt + i]) for i, b in enumerate(S.vision_blocks)}
    vpt = S.model.visual.VPT.detach().double().cpu().requires_grad_(True) if S.n_vpt else None
    octx = S.ctx.detach().double().cpu().requires_grad_(True) if S.ctx is not None else None
    return sd64, tl, vl, vpt, octx


def _drops(S, seed, blocks, width, seq, n, stream0, row0=0):
    """Dropout multipliers of the adapted blocks: the attention adapters at stream0 + 4 l + s, c_fc at
    stream0 + 500 + 2 l over ``width`` columns, c_proj at stream0 + 500 + 2 l + 1 over 4 ``width`` columns; element
    (global token row, column).  The oracle is sequence-first [L, N, d]."""
    from oracle import clip_oracle as O
    if S.p == 0:
        return None
    out = {}
    for l in blocks:
        d = {}
        for tok in S.params:
            if tok in ATTN:
                stream, cols = stream0 + 4 * l + "qkvo".index(tok), width
            else:
                stream, cols = stream0 + 500 + 2 * l + MLP.index(tok), width * (4 if tok == "c_proj" else 1)
            keep = O.dropout_keep_mask(seed, stream, row0 + n * seq, cols, S.p)[row0:]
            d[_oname(tok)] = (torch.from_numpy(keep).double() / (1 - S.p)).reshape(n, seq, cols).permute(1, 0, 2)
        out[l] = d
    return out


def _oracle_loss(S, state, img, cap, tgt, seed):
    from oracle import clip_oracle as O
    sd64, tl, vl, vpt, octx = state
    cfg = S.cfg
    B, Cn = img.shape[0], cap.shape[0]
    s = O.lora_scaling(1, S.r)
    td = _drops(S, seed, S.text_blocks, cfg.transformer_width, cfg.context_length, Cn, 0)
    vd = _drops(S, seed, S.vision_blocks, cfg.vision_width, S.model.visual.tokens, B, 1000)
    if octx is None:
        emb = O.encode_text(sd64, cap, tl, s, drops=td)
    else:
        emb = O.encode_text(sd64, cap, tl, s, embeds=O.build_prompts(octx, sd64["token_embedding.weight"], cap), drops=td)
    txt = O.class_text_features(emb, list(range(Cn)), Cn)
    fi = O.encode_image(sd64, img.double(), vl, s, vpt=vpt, drops=vd)
    logits = O.train_logits(fi, txt)
    return O.jt_cross_entropy(logits, tgt), logits


def _slot(S, layer, tok, which):
    """The trainer's gradient slot of one adapter tensor."""
    m = getattr(layer, _oname(tok))
    prm = getattr(m, which)
    if tok in MLP:
        return prm.grad_slot
    return dict((id(q), g) for q, g in layer.trainable_pairs())[id(prm)]


def _check_adapter_grads(S, state, frozen=()):
    """Every adapter gradient slot against the oracle's leaf gradient: 1e-4 of the largest gradient entry.  ``frozen``:
    (list index, token) pairs left out."""
    _, tl, vl, _, _ = state
    blocks = list(tl.values()) + list(vl.values())
    leaves = [(i, tok, nm, blocks[i][_oname(tok)][nm]) for i in range(len(S.layers)) for tok in S.params
              for nm in ("w_lora_A", "w_lora_B") if (i, tok) not in frozen]
    gmax = max(t.grad.abs().max().item() for _, _, _, t in leaves)
    worst, small = 0.0, 1e9
    for i, tok, nm, t in leaves:
        worst = max(worst, _err(_slot(S, S.layers[i], tok, nm), t.grad))
        small = min(small, t.grad.abs().max().item())
    print(f"adapter gradients: worst err {worst:.3e}, largest entry {gmax:.3e}, smallest tensor max {small:.3e}")
    assert small > 0, "an adapter without gradient: the test would be vacuous"
    assert worst < 1e-4 * max(gmax, 1e-3), f"LoRA grad err {worst:.3e} vs scale {gmax:.3e}"
    return gmax


# ---------------------------------------------------------------------------------------------------------------------
# 4. one trainer step against fp64 autograd
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prompts", [False, True], ids=["plain", "ctx+vpt"])
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("params", [("c_fc", "c_proj"), ALL6, ("q", "v", "c_proj")], ids=lambda v: "-".join(v))
@pytest.mark.parametrize("cfg_name", ["TINY", "SMALL"])
def test_train_step_against_fp64(dev, monkeypatch, cfg_name, params, p, prompts):
    from clipfs.engine import _mix_seed
    from oracle import clip_oracle as O
    monkeypatch.setattr(O, "resblock_forward", _resblock)
    S = _make(dev, cfg_name, params, p=p, n_vpt=4 if prompts else 0, with_ctx=prompts)
    img, cap, tgt = _batch(S.cfg)
    B = img.shape[0]
    S.model.train()
    tr = S.L.LoRATrainer(S.model, prompt_ctx=S.ctx)
    tr.flat.zero_grad()
    loss_sum, correct, logits = tr.forward_backward(img.to(dev), cap.to(dev), tgt.to(dev))
    seed = _mix_seed(S.model.engine.seed_base, S.model.engine.step)
    state = _oracle_state(S)
    loss, wlogits = _oracle_loss(S, state, img, cap, tgt, seed)
    loss.backward()
    print(f"logits err {_err(logits, wlogits):.3e}, loss err {abs(loss_sum.item() / B - loss.item()):.3e}")
    assert _err(logits, wlogits) < 1e-3
    assert abs(loss_sum.item() / B - loss.item()) < 1e-4
    assert correct.item() == int((wlogits.argmax(1) == tgt).sum())
    _check_adapter_grads(S, state)
    if prompts:
        _, _, _, vpt, octx = state
        assert _err(S.ctx.grad_slot, octx.grad) < 1e-4 * max(octx.grad.abs().max().item(), 1e-3)
        assert _err(S.model.visual.VPT.grad_slot, vpt.grad) < 1e-4 * max(vpt.grad.abs().max().item(), 1e-3)
    # the adapters matter: without them the logits move by far more than the bound
    with torch.no_grad():
        zero = [(i, {k: {n: np.zeros_like(v) if n == "w_lora_B" and k in MLP else v for n, v in ab.items()}
                     for k, ab in w.items()}) for i, w in enumerate(S.weights)]
        S0 = types.SimpleNamespace(**{**vars(S), "weights": [w for _, w in zero]})
        _, l0 = _oracle_loss(S0, _oracle_state(S0), img, cap, tgt, seed)
    assert _err(l0, wlogits) > 1e-2, "MLP adapters must change the logits (test is vacuous otherwise)"


def test_train_step_bf16x3(dev, monkeypatch):
    """The bf16x3 mode with every adapter: logits within 1e-3 of the fp64 oracle, gradients within 3e-3 of the largest
    entry of the exact-fp32 engine's (the bounds of test_engine_gpu.test_bf16x3_precision_mode)."""
    from clipfs.engine import _mix_seed
    from oracle import clip_oracle as O
    monkeypatch.setattr(O, "resblock_forward", _resblock)
    S = _make(dev, "SMALL", ALL6, p=0.25)
    img, cap, tgt = _batch(S.cfg)
    S.model.train()
    tr = S.L.LoRATrainer(S.model)
    res = {}
    for mode in ("fp32", "bf16x3"):
        S.model.engine.precision = mode
        S.model.engine.step = 3  # the same masks in both modes
        tr.flat.zero_grad()
        _, _, logits = tr.forward_backward(img.to(dev), cap.to(dev), tgt.to(dev))
        res[mode] = (logits.clone(), tr.flat.grads.clone())
    seed = _mix_seed(S.model.engine.seed_base, S.model.engine.step)
    with torch.no_grad():
        _, wl = _oracle_loss(S, _oracle_state(S), img, cap, tgt, seed)
    e32, e16 = _err(res["fp32"][0], wl), _err(res["bf16x3"][0], wl)
    g32, g16 = res["fp32"][1], res["bf16x3"][1]
    print(f"logits err fp32 {e32:.3e} bf16x3 {e16:.3e}; grad diff {(g32 - g16).abs().max().item():.3e} of {g32.abs().max().item():.3e}")
    assert e32 < 1e-4 and e16 < 1e-3, (e32, e16)
    assert not torch.equal(res["fp32"][0], res["bf16x3"][0])  # the mode really switched
    assert (g32 - g16).abs().max() < 3e-3 * g32.abs().max()


# ---------------------------------------------------------------------------------------------------------------------
# 5. three optimiser steps
# ---------------------------------------------------------------------------------------------------------------------

def test_three_step_trajectory(dev, monkeypatch):
    from clipfs.engine import _mix_seed
    from oracle import clip_oracle as O
    monkeypatch.setattr(O, "resblock_forward", _resblock)
    S = _make(dev, "TINY", ("q", "v", "c_fc", "c_proj"), p=0.25, with_ctx=True)
    img, cap, tgt = _batch(S.cfg)
    B = img.shape[0]
    S.model.train()
    lr = 1e-2  # large enough that three steps move the parameters well above fp32 noise
    tr = S.L.LoRATrainer(S.model, prompt_ctx=S.ctx, lr=lr)
    state = _oracle_state(S)
    _, tl, vl, _, octx = state
    blocks = list(tl.values()) + list(vl.values())
    leaves = [t for blk in blocks for ab in blk.values() for t in ab.values()] + [octx]
    start = [t.detach().clone() for t in leaves]
    mom = [(torch.zeros_like(t), torch.zeros_like(t)) for t in leaves]
    for step in range(1, 4):
        loss_sum, _, _ = tr.step(img.to(dev), cap.to(dev), tgt.to(dev))
        seed = _mix_seed(S.model.engine.seed_base, S.model.engine.step)
        for t in leaves:
            t.grad = None
        loss, _ = _oracle_loss(S, state, img, cap, tgt, seed)
        loss.backward()
        assert abs(loss_sum.item() / B - loss.item()) < 2e-4, (step, loss_sum.item() / B, loss.item())
        with torch.no_grad():
            for i, t in enumerate(leaves):
                new, m, v = O.jt_adamw_step(t.detach(), t.grad, mom[i][0], mom[i][1], step, lr=lr)
                t.copy_(new)
                mom[i] = (m, v)
    worst = _err(S.ctx, octx)
    for i, layer in enumerate(S.layers):
        for tok in S.params:
            for nm in ("w_lora_A", "w_lora_B"):
                worst = max(worst, _err(getattr(getattr(layer, _oname(tok)), nm), blocks[i][_oname(tok)][nm]))
    moved = max((a.detach() - b).abs().max().item() for a, b in zip(leaves, start))
    moved_mlp = max((blocks[0][tok][nm].detach() - torch.from_numpy(S.weights[0][tok][nm]).double()).abs().max().item()
                    for tok in MLP for nm in ("w_lora_A", "w_lora_B"))
    print(f"trajectory: worst {worst:.3e}, moved {moved:.3e}, MLP adapters moved {moved_mlp:.3e}")
    assert moved > 1e-2 and moved_mlp > 1e-2 and worst < 2e-4, (moved, moved_mlp, worst)


# ---------------------------------------------------------------------------------------------------------------------
# 6. placement, 7. freezing, 8. biases, 9. fp16, 11. autograd
# ---------------------------------------------------------------------------------------------------------------------

def test_placement_floor_and_pruning(dev, monkeypatch):
    """encoder='vision', blocks 1 and 2 of 3, MLP adapters only: the floor sits at block 1, the text tower gets no backward,
    and the gradients are bitwise those of the full-depth walk -- and the oracle's."""
    from clipfs.engine import _mix_seed
    from oracle import clip_oracle as O
    monkeypatch.setattr(O, "resblock_forward", _resblock)
    S = _make(dev, "SMALL", ("c_fc", "c_proj"), p=0.25, encoder="vision", vision_blocks=[1, 2])
    img, cap, tgt = _batch(S.cfg)
    S.model.train()
    tr = S.L.LoRATrainer(S.model)
    out = {}
    for prune in (True, False):
        S.model.engine.prune_backward = prune
        S.model.engine.step = 5
        tr.flat.zero_grad()
        _, _, logits = tr.forward_backward(img.to(dev), cap.to(dev), tgt.to(dev))
        out[prune] = (logits.clone(), tr.flat.grads.clone(), dict(tr.last_plan))
    assert out[True][2] == {"text": None, "vision": 1} and out[False][2] == {"text": 0, "vision": 0}
    assert torch.equal(out[True][0], out[False][0]) and torch.equal(out[True][1], out[False][1])
    assert out[True][1].abs().max().item() > 0
    S.model.engine.prune_backward = True
    S.model.engine.step = 5
    tr.flat.zero_grad()
    tr.forward_backward(img.to(dev), cap.to(dev), tgt.to(dev))
    state = _oracle_state(S)
    loss, _ = _oracle_loss(S, state, img, cap, tgt, _mix_seed(S.model.engine.seed_base, 6))
    loss.backward()
    _check_adapter_grads(S, state)


def test_frozen_mlp_adapters_of_one_block(dev, monkeypatch):
    """requires_grad_(False) on the MLP adapters of vision block 1: they stay out of the flat buffer and are bitwise
    unchanged after two optimiser steps, while they still act in the forward and pass their input gradient down (the
    other gradients match the oracle, whose leaves include the frozen values)."""
    from clipfs.engine import _mix_seed
    from oracle import clip_oracle as O
    monkeypatch.setattr(O, "resblock_forward", _resblock)
    S = _make(dev, "SMALL", ("q", "c_fc", "c_proj"), p=0.25)
    nt = len(S.text_blocks)
    frozen_layer = S.layers[nt + 1]
    for tok in MLP:
        m = getattr(frozen_layer, tok)
        m.w_lora_A.requires_grad_(False)
        m.w_lora_B.requires_grad_(False)
    before = {(tok, nm): getattr(getattr(frozen_layer, tok), nm).detach().clone() for tok in MLP for nm in ("w_lora_A", "w_lora_B")}
    img, cap, tgt = _batch(S.cfg)
    S.model.train()
    tr = S.L.LoRATrainer(S.model, lr=1e-2)
    tr.flat.zero_grad()
    _, _, logits = tr.forward_backward(img.to(dev), cap.to(dev), tgt.to(dev))
    seed = _mix_seed(S.model.engine.seed_base, S.model.engine.step)
    state = _oracle_state(S)
    loss, wl = _oracle_loss(S, state, img, cap, tgt, seed)
    loss.backward()
    assert _err(logits, wl) < 1e-3
    _check_adapter_grads(S, state, frozen={(nt + 1, "c_fc"), (nt + 1, "c_proj")})
    other = S.layers[nt].c_fc.w_lora_B.detach().clone()
    for _ in range(2):
        tr.step(img.to(dev), cap.to(dev), tgt.to(dev))
    for (tok, nm), v in before.items():
        assert torch.equal(getattr(getattr(frozen_layer, tok), nm).detach(), v), (tok, nm)
    assert not torch.equal(S.layers[nt].c_fc.w_lora_B.detach(), other)


def test_lora_only_biases_of_the_mlp_linears(dev, monkeypatch):
    """bias='lora_only' with params c_fc c_proj: exactly the two wrapped linears' biases train, and their gradients
    (slots g_b_fc / g_b_pr) match the oracle's to 1e-4 of the largest entry."""
    from clipfs.engine import _mix_seed
    from oracle import clip_oracle as O
    monkeypatch.setattr(O, "resblock_forward", _resblock)
    S = _make(dev, "SMALL", ("c_fc", "c_proj"), p=0.25, bias="lora_only")
    img, cap, tgt = _batch(S.cfg)
    S.model.train()
    tr = S.L.LoRATrainer(S.model)
    names = list(tr.flat.bias_names)
    want_names = [f"{pre}.resblocks.{i}.mlp.{tok}.bias" for pre, n in (("transformer", S.cfg.transformer_layers),
                                                                         ("visual.transformer", S.cfg.vision_layers))
                  for i in range(n) for tok in MLP]
    assert sorted(names) == sorted(want_names)
    tr.flat.zero_grad()
    tr.forward_backward(img.to(dev), cap.to(dev), tgt.to(dev))
    seed = _mix_seed(S.model.engine.seed_base, S.model.engine.step)
    state = _oracle_state(S, bias_names=names)
    loss, _ = _oracle_loss(S, state, img, cap, tgt, seed)
    loss.backward()
    _check_adapter_grads(S, state)
    named = dict(S.model.named_parameters())
    gmax = max(state[0][n].grad.abs().max().item() for n in names)
    worst = max(_err(named[n].grad_slot, state[0][n].grad) for n in names)
    print(f"bias gradients: worst err {worst:.3e}, largest entry {gmax:.3e}")
    assert gmax > 1e-4 and worst < 1e-4 * gmax, (worst, gmax)


@pytest.mark.parametrize("tok", MLP)
def test_fp16_mode_refuses_mlp_adapters(dev, tok):
    S = _make(dev, "TINY", (tok,), encoder="vision", vision_blocks=[1])
    S.model.engine.precision = "fp16"
    with pytest.raises(ValueError, match=rf"vision block 1 has a {tok} adapter"):
        S.L.LoRATrainer(S.model)
    # and the library refuses the descriptor itself, before anything is enqueued
    from clipfs._lib import ClipfsError
    img, _, _ = _batch(S.cfg)
    with pytest.raises(ClipfsError, match=rf"block 1 has a {tok} adapter"):
        with torch.no_grad():
            S.model.encode_image(img.to(dev))


def test_autograd_route_fills_param_grad(dev, monkeypatch):
    """encode_text / encode_image ... backward(): ``param.grad`` of the four MLP adapter tensors of a block (and of the
    attention adapters) equals the trainer's gradient slot."""
    from clipfs import engine as E
    S = _make(dev, "SMALL", ("q", "c_fc", "c_proj"))
    img, cap, tgt = _batch(S.cfg)
    img, cap, tgt = img.to(dev), cap.to(dev), tgt.to(dev)
    S.model.eval()
    txt = E.class_mean(S.model.encode_text(cap), cap.shape[0], 1)
    fi = E.l2_normalize(S.model.encode_image(img))
    loss = E.cross_entropy_loss(E.cosine_logits(fi, txt, 100.0), tgt)
    loss.backward()
    api = {n: p.grad.clone() for n, p in S.model.named_parameters() if "lora_" in n}
    assert len(api) == 6 * len(S.layers) and all(g.abs().max().item() > 0 for g in api.values())
    tr = S.L.LoRATrainer(S.model)
    tr.flat.zero_grad()
    ls, _, _ = tr.forward_backward(img, cap, tgt)
    assert abs(ls.item() / img.shape[0] - loss.item()) < 1e-5
    for i, layer in enumerate(S.layers):
        for tok in S.params:
            for nm in ("w_lora_A", "w_lora_B"):
                prm = getattr(getattr(layer, _oname(tok)), nm)
                name = [n for n, q in S.model.named_parameters() if q is prm][0]
                assert _err(api[name], _slot(S, layer, tok, nm)) < 1e-6, name


def test_fused_stage2_runs_frozen_mlp_adapters(dev, monkeypatch):
    """Stage2Trainer(fused=True) with applied-and-frozen adapters on q k v c_fc c_proj (dropout 0.25): the first step's loss
    and the ctx / VPT gradients are the unfused (autograd-route) trainer's, with the bounds of
    test_stage2_fused_gpu (loss 5e-5 relative, gradients 5e-4 of the largest entry) -- and the MLP adapters act.  The
    stage-2 fixture of that file is reused; apply_lora is wrapped so that it also adapts the MLP linears (B non-zero)."""
    import test_stage2_fused_gpu as T
    T._paths()
    import lora_train_vlp as L
    orig, with_mlp = L.apply_lora, [True]

    def apply_with_mlp(args, model):
        qkv = list(args.params)
        if with_mlp[0]:
            args.params = qkv + ["c_fc", "c_proj"]
        layers = orig(args, model)
        args.params = qkv  # the fixture fills the q / k / v adapters
        g = torch.Generator().manual_seed(3)
        with torch.no_grad():
            for layer in layers:
                for tok in MLP:
                    if getattr(layer, tok, None) is not None:
                        m = getattr(layer, tok)
                        m.w_lora_B.copy_(torch.randn(m.w_lora_B.shape, generator=g) * 0.05)
        return layers

    monkeypatch.setattr(L, "apply_lora", apply_with_mlp)
    res = {}
    for name, fused, mlp in (("fused", True, True), ("unfused", False, True), ("plain", True, False)):
        with_mlp[0] = mlp
        s = T._setup(dev, p=0.25, fused=fused)
        n_mlp = len([n for n, q in s.model.named_parameters() if "mlp" in n and "lora_" in n and not q.requires_grad])
        assert n_mlp == (4 * (s.cfg.transformer_layers + s.cfg.vision_layers) if mlp else 0)
        loss, _, _ = T._step(s)
        named = T._named(s)
        res[name] = (float(loss.sum().item()) if torch.is_tensor(loss) else float(loss), T._grad(s, named["ctx"]),
                     T._grad(s, named["VPT"]))
    f, u, z = res["fused"], res["unfused"], res["plain"]
    print(f"stage 2: loss {f[0]:.6f} vs {u[0]:.6f} (without MLP adapters {z[0]:.6f}), ctx grad err {_err(f[1], u[1]):.3e} of "
          f"{u[1].abs().max().item():.3e}, VPT grad err {_err(f[2], u[2]):.3e} of {u[2].abs().max().item():.3e}")
    assert abs(f[0] - u[0]) < 5e-5 * max(1.0, abs(u[0]))
    assert _err(f[1], u[1]) < 5e-4 * u[1].abs().max().item() and _err(f[2], u[2]) < 5e-4 * u[2].abs().max().item()
    assert abs(f[0] - z[0]) > 1e-3, "the frozen MLP adapters must act in the forward"


# ---------------------------------------------------------------------------------------------------------------------
# 10. data parallel
# ---------------------------------------------------------------------------------------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_trainer(dev, **kw):
    S = _make(dev, "SMALL", ("q", "v", "c_fc", "c_proj"), p=0.25, with_ctx=True)
    S.model.train()
    return S, S.L.LoRATrainer(S.model, prompt_ctx=S.ctx, **kw)


def _dp_rank(rank, world, port, out_dir):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for path in (os.path.join(root, "jittor-clip-fewshot_amd"), root, os.path.join(root, "tests")):
        if path not in sys.path:
            sys.path.insert(0, path)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    from clipfs import dist as D
    dev = torch.device("cuda:0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    S, tr = _dp_trainer(dev, shard_text=True)
    img, cap, tgt = (v.to(dev) for v in _batch(S.cfg, B=8))
    lo, hi = D.shard_bounds(img.shape[0], rank, world)
    tr.flat.zero_grad()
    loss_sum, _, _ = tr.forward_backward(img[lo:hi].contiguous(), cap, tgt[lo:hi].contiguous(), 1, img.shape[0], row_offset=lo)
    tr.optimizer_step()
    total = loss_sum.clone()
    D.allreduce_sum_(total)
    torch.cuda.synchronize()
    if rank == 0:
        np.savez(os.path.join(out_dir, "dp.npz"), grads=tr.flat.grads.cpu().numpy(), params=tr.flat.params.cpu().numpy(),
                 loss=total.cpu().numpy())
    dist.destroy_process_group()


def test_two_ranks_match_one_process(dev, tmp_path):
    """Two gloo ranks on the one device, class-sharded text, dropout 0.25: the MLP adapters' masks are indexed by the
    global row like the others, so the summed gradients are the one-process step's."""
    S, tr = _dp_trainer(dev)
    img, cap, tgt = (v.to(dev) for v in _batch(S.cfg, B=8))
    tr.flat.zero_grad()
    loss_sum, _, _ = tr.forward_backward(img, cap, tgt)
    tr.optimizer_step()
    want_g, want_p, want_loss = tr.flat.grads.cpu().numpy(), tr.flat.params.cpu().numpy(), loss_sum.item()
    mp.spawn(_dp_rank, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    z = np.load(os.path.join(str(tmp_path), "dp.npz"))
    scale = np.abs(want_g).max()
    err = np.abs(z["grads"] - want_g).max()
    print(f"two ranks: grad err {err:.3e} of {scale:.3e}")
    assert scale > 1e-5
    assert err < 2e-5 * scale + 1e-9
    assert np.abs(z["params"] - want_p).max() < 1e-6
    assert abs(float(z["loss"][0]) - want_loss) < 1e-4
