"""Bias training through the fused backward (mark_only_lora_as_trainable(model, bias='all' | 'lora_only')): the
column-sum kernel (clipfs_bias_grad), every bias gradient of a LoRATrainer step against fp64 autograd on the oracle,
the AdamW update of the flat buffer with frozen q / k / v segments left untouched, the autograd route, the data-parallel
step and the refusals.  Gradient tolerance as in test_engine_gpu: 1e-4 relative to the largest gradient entry."""
import os
import socket
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

_NAMES = {"q": "q_proj", "k": "k_proj", "v": "v_proj", "o": "proj"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _err(got, want):
    return (got.detach().double().cpu() - want.detach().double().cpu()).abs().max().item()


# ------------------------------------------------------------------------------------------------ kernel

def _colsum64(x):
    return x.double().sum(0)


@pytest.mark.parametrize("rows,cols", [(12800, 2304), (12800, 3072), (31031, 512), (31031, 2048), (1000, 771),
                                       (37, 6), (5, 64)])
def test_bias_grad_kernel_matches_fp64(dev, rows, cols):
    from clipfs import ops
    g = torch.Generator(device="cpu").manual_seed(rows + cols)
    x = torch.randn(rows, cols, generator=g).to(dev)
    out = torch.zeros(cols, device=dev)
    ops.bias_grad(x, out)
    want = _colsum64(x)
    tol = 2e-6 * x.abs().double().sum(0).max().item()
    assert _err(out, want) < tol
    # accumulate-into semantics, and two runs bitwise identical
    base = torch.randn(cols, generator=g).to(dev)
    a, b = base.clone(), base.clone()
    ops.bias_grad(x, a)
    ops.bias_grad(x, b)
    assert torch.equal(a, b)
    assert _err(a, want + base.double()) < tol + 1e-6


def test_bias_grad_kernel_leading_dim_and_segments(dev):
    from clipfs import ops
    g = torch.Generator(device="cpu").manual_seed(7)
    full = torch.randn(3001, 3 * 192 + 8, generator=g).to(dev)
    x = full[:, 4:4 + 3 * 192]  # ld > cols, 16-byte aligned start
    segs = [torch.zeros(192, device=dev), None, torch.full((192,), 0.5, device=dev)]
    ops.bias_grad(x, segs, seg_width=192)
    want = _colsum64(x)
    tol = 2e-6 * x.abs().double().sum(0).max().item()
    assert _err(segs[0], want[:192]) < tol
    assert _err(segs[2], want[384:] + 0.5) < tol
    # unaligned base (scalar loads): the same order of additions, so the same bits as the aligned float4 form
    y = full[:, 1:1 + 3 * 192]
    yc = y.contiguous()
    o1, o2 = torch.zeros(3 * 192, device=dev), torch.zeros(3 * 192, device=dev)
    ops.bias_grad(y, o1)
    ops.bias_grad(yc, o2)
    assert torch.equal(o1, o2)
    # a leading part of the rows only
    o3 = torch.zeros(3 * 192, device=dev)
    ops.bias_grad(yc, o3, rows=1000)
    assert _err(o3, _colsum64(yc[:1000])) < tol


# ------------------------------------------------------------------------------------------------ one step vs oracle

def _okey(name):
    """model parameter name -> (oracle state-dict key, q/k/v segment or None)."""
    for s, pr in enumerate(("q_proj", "k_proj", "v_proj")):
        if name.endswith(f"attn.{pr}.bias"):
            return name[:-len(f"{pr}.bias")] + "in_proj_bias", s
    if name.endswith("attn.proj.bias"):
        return name[:-len("proj.bias")] + "out_proj.bias", None
    return name, None


def _setup(dev, monkeypatch, bias, cfg=None, params=("q", "k", "v"), p=0.0, encoder="both", position="all", n_vpt=0,
           with_ctx=False, seed=11):
    import lora_train_vlp as L
    from clipfs import synth
    from jclip.model import build_model
    cfg = cfg or synth.SMALL
    sd = synth.synth_state_dict(cfg, seed=seed, perturb=True)
    model = build_model(sd, design_details={"vision_ctx": n_vpt} if n_vpt else None, device=dev)
    nt, nv = cfg.transformer_layers, cfg.vision_layers
    tb = list(range(nt)) if position == "all" else list(range(nt // 2, nt))
    vb = list(range(nv)) if position == "all" else list(range(nv // 2, nv))
    monkeypatch.setitem(L.INDEX_POSITIONS_TEXT, position, tb)
    monkeypatch.setitem(L.INDEX_POSITIONS_VISION.setdefault("small", {}), position, vb)
    args = types.SimpleNamespace(encoder=encoder, position=position, backbone="small", params=list(params), r=4, alpha=1,
                                 dropout_rate=p)
    layers = L.apply_lora(args, model)
    tb = tb if encoder in ("text", "both") else []
    vb = vb if encoder in ("vision", "both") else []
    lw = synth.synth_lora(cfg, 4, seed=5, params=params, text_blocks=tb, vision_blocks=vb)
    with torch.no_grad():
        for i, layer in enumerate(layers):
            for pr in params:
                m = getattr(layer, _NAMES[pr])
                m.w_lora_A.copy_(torch.from_numpy(lw[f"layer_{i}"][_NAMES[pr]]["w_lora_A"]))
                m.w_lora_B.copy_(torch.from_numpy(lw[f"layer_{i}"][_NAMES[pr]]["w_lora_B"]))
    L.mark_only_lora_as_trainable(model, bias)
    if n_vpt:
        model.visual.VPT.requires_grad_(True)
    ctx = torch.nn.Parameter(sd["token_embedding.weight"][[5, 6, 7, 8]].clone().to(dev)) if with_ctx else None
    return types.SimpleNamespace(L=L, cfg=cfg, sd=sd, model=model, layers=layers, lw=lw, tb=tb, vb=vb, params=params,
                                 p=p, ctx=ctx)


def _batch(cfg, B=6, Cn=9):
    from clipfs import synth
    img = synth.synth_images(B, cfg.image_resolution, seed=3)
    cap = synth.synth_captions(Cn, cfg.context_length, cfg.vocab_size, seed=4, max_len=12)
    tgt = synth.synth_labels(B, Cn, seed=2)
    return img, cap, tgt


def _oracle(S, img, cap, tgt, seed, bias_names):
    """fp64 autograd of the step: (loss, logits, {bias name: gradient})."""
    from oracle import clip_oracle as O
    cfg, p, params = S.cfg, S.p, S.params
    sd64 = {k: v.double() for k, v in S.sd.items()}
    for n in bias_names:
        sd64[_okey(n)[0]].requires_grad_(True)
    conv = lambda d: {pr: {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in ab.items()}
                      for pr, ab in d.items()}
    tl = {b: conv(S.lw[f"layer_{i}"]) for i, b in enumerate(S.tb)}
    vl = {b: conv(S.lw[f"layer_{len(S.tb) + i}"]) for i, b in enumerate(S.vb)}

    def drops(width, seq, n, blocks, stream0):
        if p == 0:
            return None
        out = {}
        for l in blocks:
            d = {}
            for s, pr in enumerate(("q", "k", "v", "o")):
                if pr in params:
                    keep = O.dropout_keep_mask(seed, stream0 + 4 * l + s, n * seq, width, p)
                    d[_NAMES[pr]] = (torch.from_numpy(keep).double() / (1 - p)).reshape(n, seq, width).permute(1, 0, 2)
            out[l] = d
        return out

    B, Cn = img.shape[0], cap.shape[0]
    vpt = None
    if S.model.visual.VPT is not None:
        vpt = S.model.visual.VPT.detach().double().cpu().requires_grad_(True)
    vtok = cfg.vision_tokens + (0 if vpt is None else vpt.shape[0])
    td = drops(cfg.transformer_width, cfg.context_length, Cn, S.tb, 0)
    vd = drops(cfg.vision_width, vtok, B, S.vb, 1000)
    s = O.lora_scaling(1, 4)
    octx = S.ctx.detach().double().cpu().requires_grad_(True) if S.ctx is not None else None
    pe = None if octx is None else O.build_prompts(octx, sd64["token_embedding.weight"], cap)
    emb = O.encode_text(sd64, cap, tl, s, embeds=pe, drops=td)
    txt = O.class_text_features(emb, list(range(Cn)), Cn)
    fi = O.encode_image(sd64, img.double(), vl, s, vpt=vpt, drops=vd)
    logits = O.train_logits(fi, txt)
    loss = O.jt_cross_entropy(logits, tgt)
    loss.backward()
    grads = {}
    for n in bias_names:
        key, seg = _okey(n)
        g = sd64[key].grad
        if seg is not None:
            w = g.shape[0] // 3
            g = g[seg * w:(seg + 1) * w]
        grads[n] = g
    return loss, logits, grads


def _check_bias_grads(S, want, bound=1e-4):
    named = dict(S.model.named_parameters())
    gmax = max(g.abs().max().item() for g in want.values())
    assert gmax > 1e-6
    worst, who = 0.0, None
    for n, g in want.items():
        e = _err(named[n].grad_slot, g)
        if e > worst:
            worst, who = e, n
    assert worst < bound * gmax, f"bias grad err {worst:.3e} ({who}) vs scale {gmax:.3e}"


def _expected_all(model):
    return [n for n, _ in model.named_parameters() if "bias" in n]


def _step(S, dev, B=6, Cn=9, sparse=True, trim=False):
    from clipfs.engine import _mix_seed
    img, cap, tgt = _batch(S.cfg, B, Cn)
    S.model.train()
    S.model.engine.sparse_backward = sparse
    S.model.engine.trim_text = trim
    tr = S.L.LoRATrainer(S.model, prompt_ctx=S.ctx)
    tr.flat.zero_grad()
    loss_sum, correct, logits = tr.forward_backward(img.to(dev), cap.to(dev), tgt.to(dev))
    torch.cuda.synchronize()
    seed = _mix_seed(S.model.engine.seed_base, S.model.engine.step)
    return tr, (img, cap, tgt), loss_sum, correct, logits, seed


@pytest.mark.parametrize("p,with_ctx,n_vpt", [(0.0, False, 0), (0.25, False, 0), (0.0, True, 0), (0.25, True, 0),
                                              (0.0, False, 4)])
def test_step_bias_all_vs_oracle(dev, monkeypatch, p, with_ctx, n_vpt):
    from oracle import clip_oracle as O
    S = _setup(dev, monkeypatch, "all", p=p, with_ctx=with_ctx, n_vpt=n_vpt)
    names = [n for n, _ in S.L.trainable_biases(S.model)]
    assert names == _expected_all(S.model) and len(names) == 8 * (S.cfg.transformer_layers + S.cfg.vision_layers) + 3
    tr, (img, cap, tgt), loss_sum, correct, logits, seed = _step(S, dev)
    B = img.shape[0]
    loss, wlogits, want = _oracle(S, img, cap, tgt, seed, names)
    assert _err(logits, wlogits) < 1e-3
    assert abs(loss_sum.item() / B - loss.item()) < 1e-4
    assert correct.item() == int((wlogits.argmax(1) == tgt).sum())
    assert torch.equal(S.L.ops.topk(logits, 5).cpu().long(), O.jt_topk(wlogits.float(), 5))
    _check_bias_grads(S, want)
    # the adapters' (and prompt / VPT) gradients are bit-for-bit those of the same step with bias='none'
    S0 = _setup(dev, monkeypatch, "none", p=p, with_ctx=with_ctx, n_vpt=n_vpt)
    tr0 = _step(S0, dev)[0]
    assert tr0.flat.numel == tr.flat.bias_offset
    assert torch.equal(tr0.flat.grads, tr.flat.grads[:tr.flat.bias_offset])


def test_lora_only_trains_the_wrapped_biases(dev, monkeypatch):
    from clipfs.engine import _mix_seed
    from oracle import clip_oracle as O
    S = _setup(dev, monkeypatch, "lora_only", params=("q", "v"))
    names = [n for n, _ in S.L.trainable_biases(S.model)]
    assert names and all(n.endswith(("q_proj.bias", "v_proj.bias")) for n in names)
    assert len(names) == 2 * (S.cfg.transformer_layers + S.cfg.vision_layers)
    before = {n: t.detach().clone() for n, t in S.model.state_dict().items() if "bias" in n}
    packed0 = [l.qkv_bias.detach().clone() for l in S.layers]
    img, cap, tgt = _batch(S.cfg)
    S.model.train()
    tr = S.L.LoRATrainer(S.model, weight_decay=1e-2)
    named = dict(S.model.named_parameters())
    off = tr.flat.bias_offset
    p_ref = tr.flat.params.detach().double().cpu()
    m_ref, v_ref = torch.zeros_like(p_ref), torch.zeros_like(p_ref)
    for step in range(1, 4):
        tr.flat.zero_grad()
        tr.forward_backward(img.to(dev), cap.to(dev), tgt.to(dev))
        torch.cuda.synchronize()
        # this step's oracle at the CURRENT parameters: the trained biases and adapters written back into the oracle
        S.sd = {k: v.clone() for k, v in S.sd.items()}
        for n in names:
            key, seg = _okey(n)
            w = S.sd[key].shape[0] // 3
            S.sd[key][seg * w:(seg + 1) * w] = named[n].detach().cpu()
        S.lw = {f"layer_{i}": {_NAMES[pr]: {"w_lora_A": getattr(l, _NAMES[pr]).w_lora_A.detach().cpu().numpy(),
                                            "w_lora_B": getattr(l, _NAMES[pr]).w_lora_B.detach().cpu().numpy()}
                               for pr in S.params} for i, l in enumerate(S.layers)}
        _, _, want = _oracle(S, img, cap, tgt, _mix_seed(S.model.engine.seed_base, S.model.engine.step), names)
        _check_bias_grads(S, want)
        g = tr.flat.grads.detach().double().cpu()
        g[off:] = torch.cat([want[n].reshape(-1) for n in names])  # the biases: the ORACLE's gradients
        tr.optimizer_step()
        p_ref, m_ref, v_ref = O.jt_adamw_step(p_ref, g, m_ref, v_ref, step, weight_decay=1e-2)
        assert _err(tr.flat.params[off:], p_ref[off:]) < 1e-6
    after = S.model.state_dict()
    for n, t in before.items():
        if n in names:
            assert not torch.equal(after[n], t), n
        else:
            assert torch.equal(after[n], t), f"{n} is frozen but changed"
    # the packed in-projection bias the QKV GEMM reads: trained q / v segments, k bit-for-bit the original
    for l, p0 in zip(S.layers, packed0):
        d = l.embed_dim
        assert torch.equal(l.qkv_bias[d:2 * d], p0[d:2 * d])
        assert torch.equal(l.qkv_bias[:d], l.q_proj.bias) and torch.equal(l.qkv_bias[2 * d:], l.v_proj.bias)


@pytest.mark.parametrize("encoder,position", [("both", "up"), ("vision", "all")])
def test_partial_placement(dev, monkeypatch, encoder, position):
    S = _setup(dev, monkeypatch, "all", encoder=encoder, position=position, p=0.25)
    names = [n for n, _ in S.L.trainable_biases(S.model)]
    assert names == _expected_all(S.model)
    tr, (img, cap, tgt), _, _, logits, seed = _step(S, dev)
    _, wlogits, want = _oracle(S, img, cap, tgt, seed, names)
    assert _err(logits, wlogits) < 1e-3
    _check_bias_grads(S, want)


def test_backward_variants_agree(dev, monkeypatch):
    grads = {}
    for key, sparse, trim in (("sparse", True, False), ("dense", False, False), ("trim", True, True)):
        S = _setup(dev, monkeypatch, "all", with_ctx=True)
        tr = _step(S, dev, sparse=sparse, trim=trim)[0]
        grads[key] = tr.flat.grads[tr.flat.bias_offset:].detach().cpu()
    scale = grads["sparse"].abs().max().item()
    assert (grads["dense"] - grads["sparse"]).abs().max().item() < 1e-5 * scale
    assert (grads["trim"] - grads["sparse"]).abs().max().item() < 1e-5 * scale


def test_autograd_route(dev, monkeypatch):
    """encode_image / encode_text with trainable biases: ``param.grad`` is the oracle's gradient, with two grad-enabled
    text forwards (two caption chunks) before one backward."""
    from clipfs import engine as E
    from oracle import clip_oracle as O
    S = _setup(dev, monkeypatch, "all")
    model = S.model
    model.eval()
    img, cap, tgt = _batch(S.cfg)
    ft = torch.cat([model.encode_text(cap[:4].to(dev)), model.encode_text(cap[4:].to(dev))])
    fi = model.encode_image(img.to(dev))
    logits = E.cosine_logits(E.l2_normalize(fi), E.l2_normalize(ft), 100.0)
    E.cross_entropy_loss(logits, tgt.to(dev)).backward()
    names = [n for n, _ in S.L.trainable_biases(model)]
    _, wlogits, want = _oracle(S, img, cap, tgt, 0, names)
    assert _err(logits, wlogits) < 1e-3
    named = dict(model.named_parameters())
    gmax = max(g.abs().max().item() for g in want.values())
    worst = max(_err(named[n].grad, want[n]) for n in names)
    assert worst < 1e-4 * gmax, (worst, gmax)


def test_full_width_vit_b32(dev, monkeypatch):
    from clipfs import synth
    S = _setup(dev, monkeypatch, "all", cfg=synth.VIT_B32)
    names = [n for n, _ in S.L.trainable_biases(S.model)]
    tr, (img, cap, tgt), _, _, logits, seed = _step(S, dev, B=8, Cn=16)
    _, wlogits, want = _oracle(S, img, cap, tgt, seed, names)
    assert _err(logits, wlogits) < 1e-3
    _check_bias_grads(S, want)


# ------------------------------------------------------------------------------------------------ refusals

def test_fp16_storage_mode_refuses_bias_slots(dev, monkeypatch):
    S = _setup(dev, monkeypatch, "all")
    S.model.engine.precision = "fp16"
    with pytest.raises(ValueError, match="fp16"):
        S.L.LoRATrainer(S.model)
    # a trainer built before the switch: the C driver refuses the descriptor
    S = _setup(dev, monkeypatch, "all")
    tr = S.L.LoRATrainer(S.model)
    S.model.engine.precision = "fp16"
    img, cap, tgt = _batch(S.cfg)
    with pytest.raises(Exception, match="fp16"):
        tr.forward_backward(img.to(dev), cap.to(dev), tgt.to(dev))


def test_flagged_weight_is_refused(dev, monkeypatch):
    S = _setup(dev, monkeypatch, "all")
    S.model.transformer.resblocks[1].ln_1.weight.requires_grad_(True)
    with pytest.raises(ValueError, match=r"transformer\.resblocks\.1\.ln_1\.weight"):
        S.L.LoRATrainer(S.model)


# ------------------------------------------------------------------------------------------------ data parallel

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _MP:
    """monkeypatch stand-in for the spawned ranks (setitem only)."""

    def setitem(self, d, k, v):
        d[k] = v


def _dp_setup(dev, monkeypatch):
    S = _setup(dev, monkeypatch, "all", with_ctx=True)
    S.model.train()
    img, cap, tgt = _batch(S.cfg, B=8, Cn=9)
    return S, img.to(dev), cap.to(dev), tgt.to(dev)


def _dp_rank(rank, world, port, shard_text, out_dir):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for path in (os.path.join(root, "jittor-clip-fewshot_amd"), root):
        if path not in sys.path:
            sys.path.insert(0, path)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    from clipfs import dist as D
    dev = torch.device("cuda:0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    S, img, cap, tgt = _dp_setup(dev, _MP())  # a process of its own: the patched position tables die with it
    tr = S.L.LoRATrainer(S.model, prompt_ctx=S.ctx, shard_text=shard_text)
    lo, hi = D.shard_bounds(img.shape[0], rank, world)
    tr.flat.zero_grad()
    tr.forward_backward(img[lo:hi].contiguous(), cap, tgt[lo:hi].contiguous(), 1, img.shape[0], row_offset=lo)
    tr.optimizer_step()
    torch.cuda.synchronize()
    if rank == 0:
        np.savez(os.path.join(out_dir, "dp.npz"), grads=tr.flat.grads.cpu().numpy(), params=tr.flat.params.cpu().numpy(),
                 off=tr.flat.bias_offset)
    dist.destroy_process_group()


@pytest.mark.parametrize("shard_text", [False, True])
def test_two_ranks_bias_gradients(dev, tmp_path, monkeypatch, shard_text):
    S, img, cap, tgt = _dp_setup(dev, monkeypatch)
    tr = S.L.LoRATrainer(S.model, prompt_ctx=S.ctx)
    tr.flat.zero_grad()
    tr.forward_backward(img, cap, tgt)
    tr.optimizer_step()
    want_g, want_p = tr.flat.grads.cpu().numpy(), tr.flat.params.cpu().numpy()
    mp.spawn(_dp_rank, args=(2, _free_port(), shard_text, str(tmp_path)), nprocs=2, join=True)
    z = np.load(os.path.join(str(tmp_path), "dp.npz"))
    off = int(z["off"])
    assert off == tr.flat.bias_offset
    scale = np.abs(want_g[off:]).max()
    assert scale > 1e-6
    assert np.abs(z["grads"][off:] - want_g[off:]).max() < 2e-5 * scale
    # AdamW's first step moves every entry by ~lr * sign(g): where the gradient is rounding noise around an exact zero
    # (a key bias shifts every logit of a softmax row alike, so d loss / d k_proj.bias = 0) the sign is the noise's
    live = np.abs(want_g) > 1e-3 * scale
    assert np.abs(z["params"] - want_p)[live].max() < 1e-6
    assert np.abs(z["params"] - want_p).max() < 2 * 2e-4 + 1e-6
