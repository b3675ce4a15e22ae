"""Adapter placement (--encoder / --position) and frozen adapters through the fused backward: the gradient floor
(clipfs_tower.grad_lo, Engine.prune_backward) and the dx-only LoRA backward (NULL dA / dB).

A 6-layer synthetic model makes bottom / mid / up / half-up distinct.  Budgets are those of
test_engine_gpu.test_train_step_gradients (logits 1e-3, loss 1e-4, gradients 1e-4 relative); pruned vs unpruned is
bitwise."""
import ctypes
import os
import socket
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

POS6 = {"bottom": [0, 1], "mid": [2, 3], "up": [4, 5], "half-up": [3, 4, 5], "all": [0, 1, 2, 3, 4, 5]}
NAMES = {"q": "q_proj", "k": "k_proj", "v": "v_proj", "o": "proj"}


def _cfg6():
    from clipfs import synth
    return synth.ClipConfig("six", 128, 96, 6, 192, 32, 24, 1024, 128, 6)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _adapted(encoder, position):
    """(tower, block) of every adapter in apply_lora order (text blocks first)."""
    out = []
    if encoder in ("text", "both"):
        out += [("text", b) for b in POS6[position]]
    if encoder in ("vision", "both"):
        out += [("vision", b) for b in POS6[position]]
    return out


def _make(dev, encoder, position, p=0.0, params=("q", "k", "v"), n_vpt=0, with_ctx=False, freeze_text=False,
          freeze_all=False):
    """6-layer model with adapters at ``position`` of the ``encoder`` towers; the position tables are patched to the
    6-layer depth for the apply_lora call (as test_engine_gpu._apply does)."""
    import lora_train_vlp as L
    from clipfs import synth
    from jclip.model import build_model
    cfg = _cfg6()
    sd = synth.synth_state_dict(cfg, seed=11, perturb=True)
    model = build_model(sd, design_details={"vision_ctx": n_vpt} if n_vpt else None, device=dev)
    args = types.SimpleNamespace(encoder=encoder, position=position, backbone="six", params=list(params), r=4, alpha=1,
                                 dropout_rate=p)
    old_t = L.INDEX_POSITIONS_TEXT.get(position)
    L.INDEX_POSITIONS_TEXT[position] = POS6[position]
    L.INDEX_POSITIONS_VISION["six"] = {position: POS6[position]}
    try:
        layers = L.apply_lora(args, model)
    finally:
        if old_t is None:
            del L.INDEX_POSITIONS_TEXT[position]
        else:
            L.INDEX_POSITIONS_TEXT[position] = old_t
        del L.INDEX_POSITIONS_VISION["six"]
    lw = synth.synth_lora(cfg, 4, seed=5, params=params)  # layer_b: text block b, layer_{6+b}: vision block b
    where = _adapted(encoder, position)
    assert len(where) == len(layers)
    with torch.no_grad():
        for layer, (tw, b) in zip(layers, where):
            ab = lw[f"layer_{b if tw == 'text' else 6 + b}"]
            for pr in params:
                m = getattr(layer, NAMES[pr])
                m.w_lora_A.copy_(torch.from_numpy(ab[NAMES[pr]]["w_lora_A"]))
                m.w_lora_B.copy_(torch.from_numpy(ab[NAMES[pr]]["w_lora_B"]))
    L.mark_only_lora_as_trainable(model)
    for layer, (tw, _) in zip(layers, where):
        if freeze_all or (freeze_text and tw == "text"):
            for prm, _ in layer.trainable_pairs():
                prm.requires_grad_(False)
    if n_vpt:
        model.visual.VPT.requires_grad_(True)
    ctx = torch.nn.Parameter(sd["token_embedding.weight"][[5, 6, 7, 8]].clone().to(dev)) if with_ctx else None
    B, Cn = 6, 9
    img = synth.synth_images(B, cfg.image_resolution, seed=3).to(dev)
    cap = synth.synth_captions(Cn, cfg.context_length, cfg.vocab_size, seed=4, max_len=12).to(dev)
    tgt = synth.synth_labels(B, Cn, seed=2).to(dev)
    return types.SimpleNamespace(L=L, cfg=cfg, sd=sd, model=model, layers=layers, where=where, lw=lw, ctx=ctx, img=img,
                                 cap=cap, tgt=tgt, p=p, params=params)


def _oracle(s, seed, frozen=(), vpt=None):
    """fp64 autograd on the oracle fed only the adapted blocks; ``frozen`` towers' adapters are constants."""
    from oracle import clip_oracle as O
    cfg, p = s.cfg, s.p
    sd64 = {k: v.double() for k, v in s.sd.items()}
    tl, vl = {}, {}
    for tw, b in s.where:
        ab = s.lw[f"layer_{b if tw == 'text' else 6 + b}"]
        rg = tw not in frozen
        d = {pr: {k: torch.from_numpy(v).double().requires_grad_(rg) for k, v in w.items()} for pr, w in ab.items()}
        (tl if tw == "text" else vl)[b] = d

    def drops(adapted, width, seq, n, stream0):
        if p == 0 or not adapted:
            return None
        out = {}
        for l in adapted:
            out[l] = {}
            for k, pr in enumerate(("q", "k", "v", "o")):
                if pr in s.params:
                    keep = O.dropout_keep_mask(seed, stream0 + 4 * l + k, n * seq, width, p)
                    m = torch.from_numpy(keep).double() / (1 - p)
                    out[l][NAMES[pr]] = m.reshape(n, seq, width).permute(1, 0, 2)
        return out

    B, Cn = s.img.shape[0], s.cap.shape[0]
    td = drops(sorted(tl), cfg.transformer_width, cfg.context_length, Cn, 0)
    vd = drops(sorted(vl), cfg.vision_width, cfg.vision_tokens + (0 if vpt is None else vpt.shape[0]), B, 1000)
    octx = s.ctx.detach().double().cpu().requires_grad_() if s.ctx is not None else None
    sc = O.lora_scaling(1, 4)
    cap, img, tgt = s.cap.cpu(), s.img.double().cpu(), s.tgt.cpu()
    if octx is None:
        emb = O.encode_text(sd64, cap, tl or None, sc, drops=td)
    else:
        emb = O.encode_text(sd64, cap, tl or None, sc, embeds=O.build_prompts(octx, sd64["token_embedding.weight"], cap),
                            drops=td)
    txt = O.class_text_features(emb, list(range(Cn)), Cn)
    fi = O.encode_image(sd64, img, vl or None, sc, vpt=vpt, drops=vd)
    logits = O.train_logits(fi, txt)
    loss = O.jt_cross_entropy(logits, tgt)
    loss.backward()
    return loss, logits, tl, vl, octx


def _err(got, want):
    return (got.detach().double().cpu() - want.detach().double().cpu()).abs().max().item()


def _step(s, prune=True, precision="fp32", step0=None):
    """One forward_backward on a fresh trainer state; returns (logits, flat grads, trainer)."""
    tr = s.tr if hasattr(s, "tr") else s.L.LoRATrainer(s.model, prompt_ctx=s.ctx)
    s.tr = tr
    eng = s.model.engine  # (after the trainer: building its flat buffer rebuilds the engine)
    eng.prune_backward = prune
    eng.precision = precision
    if step0 is not None:
        eng.step = step0  # same dropout seed for A/B runs
    tr.flat.zero_grad()
    loss_sum, _, logits = tr.forward_backward(s.img, s.cap, s.tgt)
    torch.cuda.synchronize()
    s.loss = loss_sum.item() / s.img.shape[0]
    return logits.clone(), tr.flat.grads.clone(), tr


def _check_oracle(s, tr, logits, seed, frozen=()):
    loss, wl, tl, vl, octx = _oracle(s, seed, frozen)
    assert _err(logits, wl) < 1e-3
    assert abs(s.loss - loss.item()) < 1e-4
    grads = []
    for layer, (tw, b) in zip(s.layers, s.where):
        if tw in frozen:
            continue
        blk = (tl if tw == "text" else vl)[b]
        pairs = dict((id(prm), g) for prm, g in layer.trainable_pairs())
        for pr in s.params:
            m = getattr(layer, NAMES[pr])
            for nm, prm in (("w_lora_A", m.w_lora_A), ("w_lora_B", m.w_lora_B)):
                grads.append((pairs[id(prm)], blk[NAMES[pr]][nm].grad))
    if grads:
        gmax = max(w.abs().max().item() for _, w in grads)
        worst = max(_err(g, w) for g, w in grads)
        assert worst < 1e-4 * max(gmax, 1e-3), f"LoRA grad err {worst:.3e} vs scale {gmax:.3e}"
    if octx is not None:
        assert _err(s.ctx.grad_slot, octx.grad) < 1e-4 * max(octx.grad.abs().max().item(), 1e-3)
    return loss


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_ctx", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("position", ["bottom", "mid", "up"])
@pytest.mark.parametrize("encoder", ["text", "vision", "both"])
def test_placement_matches_oracle(dev, encoder, position, p, with_ctx):
    from clipfs.engine import _mix_seed
    s = _make(dev, encoder, position, p=p, with_ctx=with_ctx)
    s.model.train()
    logits, _, tr = _step(s)
    seed = _mix_seed(s.model.engine.seed_base, s.model.engine.step)
    lo = POS6[position][0]
    want_text = (0 if with_ctx else lo) if (encoder != "vision" or with_ctx) else None
    assert tr.last_plan == {"text": want_text, "vision": lo if encoder != "text" else None}
    _check_oracle(s, tr, logits, seed)


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("case", ["text-up", "vision-mid", "both-half-up-qkvo", "vision-up-vpt", "both-up-ctx"])
def test_pruned_equals_unpruned(dev, case, precision):
    kw = dict(p=0.25)
    if case == "text-up":
        s = _make(dev, "text", "up", **kw)
    elif case == "vision-mid":
        s = _make(dev, "vision", "mid", **kw)
    elif case == "both-half-up-qkvo":  # o adapter in the last block: the dense last-block fall-back
        s = _make(dev, "both", "half-up", params=("q", "k", "v", "o"), **kw)
    elif case == "vision-up-vpt":
        s = _make(dev, "vision", "up", n_vpt=4, **kw)
    else:
        s = _make(dev, "both", "up", with_ctx=True, **kw)
    s.model.train()
    l1, g1, tr = _step(s, prune=True, precision=precision, step0=7)
    plan = dict(tr.last_plan)
    l0, g0, tr = _step(s, prune=False, precision=precision, step0=7)
    assert tr.last_plan == {"text": 0, "vision": 0}
    assert plan != tr.last_plan
    assert torch.equal(l1, l0)
    assert torch.equal(g1, g0)
    assert g1.abs().max().item() > 0


# 3 ---------------------------------------------------------------------------------------------------------------
def test_work_is_skipped(dev):
    from clipfs import _lib
    s = _make(dev, "text", "up", p=0.25)
    s.model.train()
    _, _, tr = _step(s)
    eng = s.model.engine
    assert tr.last_plan == {"text": 4, "vision": None}
    lib = _lib.load()
    n_cap = s.cap.shape[0]

    def saved_bufs(rt):
        return [k[1] for k in rt._bufs if k[0] == "saved"]

    want = lib.clipfs_tower_saved_floats(ctypes.byref(eng.txt.descriptor(True, 1, None, 0, 4)), n_cap)
    full = lib.clipfs_tower_saved_floats(ctypes.byref(eng.txt.descriptor(True, 1, None, 0, 0)), n_cap)
    assert want * 6 == full * 2
    assert saved_bufs(eng.txt) == [want]
    assert saved_bufs(eng.vis) == []  # the image tower ran its no-grad forward: nothing saved, no backward
    # the flat buffer holds the text adapters only
    assert tr.flat.numel == sum(p.numel() for layer in s.layers for _, p, _ in layer.stacked())


# 4 ---------------------------------------------------------------------------------------------------------------
def test_frozen_text_adapters(dev):
    from clipfs.engine import _mix_seed
    s = _make(dev, "both", "half-up", p=0.25, with_ctx=True, freeze_text=True)
    s.model.train()
    text_layers = [layer for layer, (tw, _) in zip(s.layers, s.where) if tw == "text"]
    before = [(layer.lora_A_qkv.clone(), layer.lora_B_qkv.clone()) for layer in text_layers]
    logits, _, tr = _step(s)
    seed = _mix_seed(s.model.engine.seed_base, s.model.engine.step)
    assert tr.last_plan == {"text": 0, "vision": 3}
    n_vis = sum(p.numel() for layer, (tw, _) in zip(s.layers, s.where) if tw == "vision" for _, p, _ in layer.stacked())
    assert tr.flat.numel == n_vis + s.ctx.numel()
    _check_oracle(s, tr, logits, seed, frozen=("text",))
    tr.optimizer_step()
    tr.step(s.img, s.cap, s.tgt)
    torch.cuda.synchronize()
    for layer, (a, b) in zip(text_layers, before):
        assert torch.equal(layer.lora_A_qkv, a) and torch.equal(layer.lora_B_qkv, b)


def test_mixed_freezing_in_one_block_is_refused(dev):
    s = _make(dev, "text", "up")
    s.layers[0].q_proj.w_lora_A.requires_grad_(False)
    with pytest.raises(ValueError, match="text block 4"):
        s.L.LoRATrainer(s.model)


# 5 ---------------------------------------------------------------------------------------------------------------
def test_stage2_layout(dev):
    """Every adapter frozen, VPT + prompt ctx trained (slow_pace.py:1556-1564)."""
    s = _make(dev, "both", "all", p=0.25, n_vpt=4, with_ctx=True, freeze_all=True)
    s.model.train()
    vpt = s.model.visual.VPT
    logits, _, tr = _step(s)
    assert tr.flat.numel == s.ctx.numel() + vpt.numel()
    assert tr.last_plan == {"text": 0, "vision": 0}
    from clipfs.engine import _mix_seed
    seed = _mix_seed(s.model.engine.seed_base, s.model.engine.step)
    ovpt = vpt.detach().double().cpu().requires_grad_()
    _, wl, _, _, octx = _oracle(s, seed, frozen=("text", "vision"), vpt=ovpt)
    assert _err(logits, wl) < 1e-3
    assert _err(s.ctx.grad_slot, octx.grad) < 1e-4 * max(octx.grad.abs().max().item(), 1e-3)
    assert _err(vpt.grad_slot, ovpt.grad) < 1e-4 * max(ovpt.grad.abs().max().item(), 1e-3)


def test_nothing_trainable_is_refused(dev):
    s = _make(dev, "both", "up", freeze_all=True)
    with pytest.raises(ValueError):
        s.L.LoRATrainer(s.model)


# 6 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,r,nseg,f16dy", [(768, 4, 3, False), (512, 4, 1, False), (1024, 16, 3, True),
                                                (192, 8, 3, False)])
@pytest.mark.parametrize("p", [0.0, 0.25])
def test_dx_only_lora_backward(dev, width, r, nseg, f16dy, p):
    from clipfs import ops
    g = torch.Generator(device="cpu").manual_seed(width + r)
    rows = 1000
    mk = lambda *sh: torch.randn(*sh, generator=g).to(dev)  # noqa: E731
    x, dy, A, B = mk(rows, width), mk(rows, nseg * width), mk(nseg * r, width) * 0.05, mk(nseg * width, r) * 0.05
    t = ops.lora_down(x, A, r, nseg, p=p, seed=99, stream_base=4)
    if f16dy:
        dy = dy.half().contiguous()
    dA, dB = torch.zeros_like(A), torch.zeros_like(B)
    dx1 = mk(rows, width)
    dx0 = dx1.clone()
    dt1 = ops.lora_bwd(dy, x, t, A, B, dA, dB, dx=dx1, scale=0.5, p=p, seed=99, stream_base=4)
    dt0 = ops.lora_bwd(dy, x, t, A, B, None, None, dx=dx0, scale=0.5, p=p, seed=99, stream_base=4)
    torch.cuda.synchronize()
    assert torch.equal(dt0, dt1)
    assert torch.equal(dx0, dx1)
    assert dA.abs().max().item() > 0  # the call with slots did reduce
    dt2 = ops.lora_bwd(dy, x, t, A, B, None, None, dx=None, scale=0.5, p=p, seed=99, stream_base=4)
    torch.cuda.synchronize()
    assert torch.equal(dt2, dt1)


# 7 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("encoder,position", [("text", "up"), ("vision", "mid"), ("both", "bottom")])
def test_autograd_route_matches_trainer(dev, encoder, position):
    from clipfs import engine as E
    s = _make(dev, encoder, position)
    s.model.eval()
    _, g_tr, tr = _step(s)
    want = {id(prm): g.clone() for layer in s.layers for prm, g in layer.trainable_pairs()}
    emb = s.model.encode_text(s.cap)
    txt = E.class_mean(emb, s.cap.shape[0], 1)
    fi = E.l2_normalize(s.model.encode_image(s.img))
    E.cross_entropy_loss(E.cosine_logits(fi, txt, 100.0), s.tgt).backward()
    gmax = max(w.abs().max().item() for w in want.values())
    for layer in s.layers:
        for prm, _ in layer.trainable_pairs():
            assert prm.grad is not None
            assert _err(prm.grad, want[id(prm)]) < 1e-5 * max(gmax, 1e-3)


# 8 ---------------------------------------------------------------------------------------------------------------
def _free_port():
    so = socket.socket()
    so.bind(("127.0.0.1", 0))
    port = so.getsockname()[1]
    so.close()
    return port


def _rank_main(rank, world, port, out_dir):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for path in (os.path.join(root, "jittor-clip-fewshot_amd"), root):
        if path not in sys.path:
            sys.path.insert(0, path)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    from clipfs import dist as D
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda:0")
    s = _make(dev, "vision", "up")
    s.model.eval()
    tr = s.L.LoRATrainer(s.model, shard_text=True)
    lo, hi = D.shard_bounds(s.img.shape[0], rank, world)
    tr.flat.zero_grad()
    tr.time_collectives = True
    tr.forward_backward(s.img[lo:hi].contiguous(), s.cap, s.tgt[lo:hi].contiguous(), 1, s.img.shape[0], row_offset=lo)
    tr.optimizer_step()
    torch.cuda.synchronize()
    times = tr.collective_times_ms()
    assert tr.last_plan == {"text": None, "vision": 4}
    assert tr.collectives_per_step == 2
    assert sorted(times) == ["all_gather", "all_reduce"], times
    if rank == 0:
        np.savez(os.path.join(out_dir, "dp.npz"), grads=tr.flat.grads.cpu().numpy(), params=tr.flat.params.cpu().numpy())
    dist.destroy_process_group()


def test_two_ranks_frozen_sharded_text(dev, tmp_path):
    s = _make(dev, "vision", "up")
    s.model.eval()
    _, g, tr = _step(s)
    tr.optimizer_step()
    want_g, want_p = g.cpu().numpy(), tr.flat.params.cpu().numpy()
    mp.spawn(_rank_main, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    z = np.load(os.path.join(str(tmp_path), "dp.npz"))
    scale = np.abs(want_g).max()
    assert scale > 1e-5
    assert np.abs(z["grads"] - want_g).max() < 2e-5 * scale + 1e-9
    assert np.abs(z["params"] - want_p).max() < 1e-6


# 9 ---------------------------------------------------------------------------------------------------------------
def test_vitb32_cfg2_text_up_bitwise(dev):
    """ViT-B/32 at the cfg-2 geometry (256 images, 403 captions, dropout 0.25), encoder='text', position='up'."""
    import lora_train_vlp as L
    from clipfs import synth
    from jclip.model import build_model
    cfg = synth.VIT_B32
    model = build_model(synth.synth_state_dict(cfg, seed=1234), device=dev)
    args = types.SimpleNamespace(encoder="text", position="up", backbone="ViT-B/32", params=["q", "k", "v"], r=4,
                                 alpha=1, dropout_rate=0.25)
    layers = L.apply_lora(args, model)
    lw = synth.synth_lora(cfg, 4, seed=5, text_blocks=range(4), vision_blocks=())
    with torch.no_grad():
        for i, layer in enumerate(layers):
            for pr in "qkv":
                m = getattr(layer, NAMES[pr])
                m.w_lora_A.copy_(torch.from_numpy(lw[f"layer_{i}"][NAMES[pr]]["w_lora_A"]))
                m.w_lora_B.copy_(torch.from_numpy(lw[f"layer_{i}"][NAMES[pr]]["w_lora_B"]))
    L.mark_only_lora_as_trainable(model)
    model.train()
    img = synth.synth_images(256, 224, seed=0).to(dev)
    cap = synth.synth_captions(403, 77, cfg.vocab_size, seed=1).to(dev)
    tgt = synth.synth_labels(256, 403, seed=2).to(dev)
    tr = L.LoRATrainer(model, shard_text=False)
    out = {}
    for prune in (True, False):
        model.engine.prune_backward = prune
        model.engine.step = 3
        tr.flat.zero_grad()
        _, _, logits = tr.forward_backward(img, cap, tgt)
        torch.cuda.synchronize()
        out[prune] = (logits.clone(), tr.flat.grads.clone(), dict(tr.last_plan))
    assert out[True][2] == {"text": 8, "vision": None}
    assert torch.equal(out[True][0], out[False][0])
    assert torch.equal(out[True][1], out[False][1])
