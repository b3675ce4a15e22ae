"""Deep prompts (IVLP vision_depth / language_depth, design_details["deep_prompts"]) on the GPU: the put / harvest
kernels against torch, features and gradients of every trainable tensor against an fp64 model composed from the oracle's
blocks, the engine's A/B paths, the gradient floor, the 16-bit precisions and both trainers.

The 6-layer synthetic model of test_placement_gpu; budgets of test_engine_gpu (logits 1e-3, loss 1e-4, gradients 1e-4
relative)."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

NAMES = {"q": "q_proj", "k": "k_proj", "v": "v_proj", "o": "proj"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _cfg6(context_length=24):
    from clipfs import synth
    return synth.ClipConfig("six", 128, 96, 6, 192, 32, context_length, 1024, 128, 6)


def _design(depth, deep=True):
    return {"vision_ctx": 4, "language_ctx": 4, "deep_prompts": deep, "vision_depth": depth, "language_depth": depth}


def _make(dev, depth, p=0.0, Cn=9, deep=True, with_lora=True, context_length=24, max_len=12, min_len=6):
    """6-layer model with rank-4 q/k/v adapters on every block of both towers, 4 VPT tokens, 4 ctx tokens and deep
    prompts on blocks 1 ... depth-1; LoRA, ctx, VPT and every deep prompt trainable.  Captions: SOT, min_len ... max_len
    tokens, EOT."""
    import lora_train_vlp as L
    from clipfs import synth
    from jclip.model import build_model
    cfg = _cfg6(context_length)
    sd = synth.synth_state_dict(cfg, seed=11, perturb=True)
    model = build_model(sd, design_details=_design(depth, deep), device=dev)
    layers = []
    if with_lora:
        args = types.SimpleNamespace(encoder="both", position="all", backbone="six", params=["q", "k", "v"], r=4, alpha=1,
                                     dropout_rate=p)
        old = L.INDEX_POSITIONS_TEXT["all"]
        L.INDEX_POSITIONS_TEXT["all"] = list(range(6))
        L.INDEX_POSITIONS_VISION["six"] = {"all": list(range(6))}
        try:
            layers = L.apply_lora(args, model)
        finally:
            L.INDEX_POSITIONS_TEXT["all"] = old
            del L.INDEX_POSITIONS_VISION["six"]
        lw = synth.synth_lora(cfg, 4, seed=5)
        with torch.no_grad():
            for i, layer in enumerate(layers):
                for pr in "qkv":
                    m = getattr(layer, NAMES[pr])
                    m.w_lora_A.copy_(torch.from_numpy(lw[f"layer_{i}"][NAMES[pr]]["w_lora_A"]))
                    m.w_lora_B.copy_(torch.from_numpy(lw[f"layer_{i}"][NAMES[pr]]["w_lora_B"]))
    L.mark_only_lora_as_trainable(model)
    model.visual.VPT.requires_grad_(True)
    for n, prm in model.named_parameters():
        if n.endswith(".VPT_shallow"):
            prm.requires_grad_(True)
    ctx = torch.nn.Parameter(sd["token_embedding.weight"][[5, 6, 7, 8]].clone().to(dev))
    B = 6
    img = synth.synth_images(B, cfg.image_resolution, seed=3).to(dev)
    cap = synth.synth_captions(Cn, cfg.context_length, cfg.vocab_size, seed=4, min_len=min_len, max_len=max_len).to(dev)
    tgt = synth.synth_labels(B, Cn, seed=2).to(dev)
    return types.SimpleNamespace(L=L, cfg=cfg, sd=sd, model=model, layers=layers, ctx=ctx, img=img, cap=cap, tgt=tgt)


def _deep(model):
    """{tower: {block: VPT_shallow}}"""
    return {tw: {i: b.VPT_shallow for i, b in enumerate(t.resblocks) if b.VPT_shallow is not None}
            for tw, t in (("text", model.transformer), ("vision", model.visual.transformer))}


def _err(got, want):
    return (got.detach().double().cpu() - want.detach().double().cpu()).abs().max().item()


def _step(s, step0=1, **flags):
    """One forward_backward (trainer kept on ``s``) with engine ``flags``; returns (logits, flat grads)."""
    tr = getattr(s, "tr", None) or s.L.LoRATrainer(s.model, prompt_ctx=s.ctx)
    s.tr = tr
    eng = s.model.engine
    for k, v in dict(dict(sparse_backward=True, prune_backward=True, pack_text_backward=True, pack_text_forward=True,
                          precision="fp32"), **flags).items():
        setattr(eng, k, v)
    eng.step = step0  # the same dropout seed for every A/B leg
    tr.flat.zero_grad()
    loss_sum, _, logits = tr.forward_backward(s.img, s.cap, s.tgt)
    torch.cuda.synchronize()
    s.loss = loss_sum.item() / s.img.shape[0]
    return logits.clone(), tr.flat.grads.clone()


# ---- fp64 reference: the oracle's blocks with the IVLP row replacement (model1.py:95-116) ----------------------------
def _tower64(x, sd64, prefix, heads, mask, lora, sc, prompts, tail):
    from oracle import clip_oracle as O
    for i in range(O.count_layers(sd64, prefix)):
        if i in prompts:
            pr = prompts[i]
            n, L = pr.shape[0], x.shape[0]
            f = L - n if tail else 1
            x = torch.cat([x[:f], pr.unsqueeze(1).expand(n, x.shape[1], -1), x[f + n:]], dim=0)
        x = O.resblock_forward(x, O._block_params(sd64, prefix, i), heads, mask, lora.get(i), sc, None)
    return x


def _oracle(s):
    from oracle import clip_oracle as O
    from clipfs import synth
    cfg = s.cfg
    sd64 = {k: v.double() for k, v in s.sd.items()}
    lw = synth.synth_lora(cfg, 4, seed=5)
    lora = {}
    for i in range(12):
        lora[i] = {NAMES[pr]: {k: torch.from_numpy(v).double().requires_grad_() for k, v in lw[f"layer_{i}"][NAMES[pr]].items()}
                   for pr in "qkv"}
    tl = {b: lora[b] for b in range(6)}
    vl = {b: lora[6 + b] for b in range(6)}
    deep = {tw: {i: p.detach().double().cpu().requires_grad_() for i, p in d.items()} for tw, d in _deep(s.model).items()}
    ctx = s.ctx.detach().double().cpu().requires_grad_()
    vpt = s.model.visual.VPT.detach().double().cpu().requires_grad_()
    sc = O.lora_scaling(1, 4)
    cap, img, tgt = s.cap.cpu(), s.img.double().cpu(), s.tgt.cpu()
    # text (O.encode_text with the prompt embeddings)
    x = O.build_prompts(ctx, sd64["token_embedding.weight"], cap) + sd64["positional_embedding"]
    x = x.permute(1, 0, 2)
    x = _tower64(x, sd64, "transformer", cfg.transformer_width // 64, O.build_causal_mask(x.shape[0], x.dtype), tl, sc,
                 deep["text"], tail=False).permute(1, 0, 2)
    x = O.jt_layer_norm(x, sd64["ln_final.weight"], sd64["ln_final.bias"])
    emb = x[torch.arange(x.shape[0]), cap.argmax(dim=-1)] @ sd64["text_projection"]
    # image (O.encode_image with the VPT tokens)
    w = sd64["visual.conv1.weight"]
    width, _, ps, _ = w.shape
    x = torch.nn.functional.conv2d(img, w, stride=ps)
    B = x.shape[0]
    x = x.reshape(B, width, -1).permute(0, 2, 1)
    x = torch.cat([sd64["visual.class_embedding"] + torch.zeros(B, 1, width, dtype=x.dtype), x], dim=1)
    x = x + sd64["visual.positional_embedding"]
    x = torch.cat([x, vpt.unsqueeze(0).expand(B, -1, -1)], dim=1)
    x = O.jt_layer_norm(x, sd64["visual.ln_pre.weight"], sd64["visual.ln_pre.bias"]).permute(1, 0, 2)
    x = _tower64(x, sd64, "visual.transformer", width // 64, None, vl, sc, deep["vision"], tail=True).permute(1, 0, 2)
    fi = O.jt_layer_norm(x[:, 0, :], sd64["visual.ln_post.weight"], sd64["visual.ln_post.bias"]) @ sd64["visual.proj"]
    txt = O.class_text_features(emb, list(range(cap.shape[0])), cap.shape[0])
    logits = O.train_logits(fi, txt)
    loss = O.jt_cross_entropy(logits, tgt)
    loss.backward()
    return loss, logits, tl, vl, deep, ctx, vpt


# 1 ---------------------------------------------------------------------------------------------------------------
def _lib():
    from clipfs import _lib as LB
    return LB.load()


def _rows(off, batch, seq, first, n, packed):
    out = {}
    for c in range(batch):
        for j in range(n):
            pos = first + j
            if packed:
                if pos < off[c + 1] - off[c]:
                    out[(c, j)] = off[c] + pos
            elif pos < seq:
                out[(c, j)] = c * seq + pos
    return out


@pytest.mark.parametrize("width", [128, 200])
@pytest.mark.parametrize("packed", [False, True])
def test_kernels_match_torch(dev, packed, width):
    from clipfs import _lib as LB
    lib = _lib()
    g = torch.Generator().manual_seed(7)
    batch, seq, first, n = 37, 24, 1, 4
    lens = torch.randint(1, seq + 1, (batch,), generator=g)
    lens[:5] = torch.tensor([1, 2, 3, 4, 5])  # EOT at or before row n: the EOT row itself is a prompt row, later ones skipped
    off = torch.zeros(batch + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(lens, 0)
    rows_total = int(off[-1]) if packed else batch * seq
    off_d = off.to(device=dev, dtype=torch.int32)
    offp = off_d.data_ptr() if packed else None
    rows = _rows(off.tolist(), batch, seq, first, n, packed)
    st = torch.cuda.current_stream().cuda_stream
    prompt = torch.randn(n, width, generator=g).to(dev)
    # put
    x = torch.randn(rows_total, width, generator=g).to(dev)
    want = x.clone()
    for (c, j), r in rows.items():
        want[r] = prompt[j]
    LB.check(lib.clipfs_prompt_put(prompt.data_ptr(), x.data_ptr(), offp, batch, seq, first, n, width, st), "put")
    torch.cuda.synchronize()
    assert torch.equal(x, want)
    # harvest (with the f16 image), twice from the same input: bitwise the same
    dx0 = torch.randn(rows_total, width, generator=g).to(dev)
    g0 = torch.randn(n, width, generator=g).to(dev)
    want_g = g0.double().clone()
    want_dx = dx0.clone()
    for (c, j), r in rows.items():
        want_g[j] += dx0[r].double()
        want_dx[r] = 0
    outs = []
    for _ in range(2):
        dx, dx16, gg = dx0.clone(), dx0.half(), g0.clone()
        LB.check(lib.clipfs_prompt_harvest(dx.data_ptr(), dx16.data_ptr(), offp, batch, seq, first, n, width, gg.data_ptr(),
                                           st), "harvest")
        torch.cuda.synchronize()
        assert torch.equal(dx, want_dx)
        assert torch.equal(dx16, want_dx.half())
        assert _err(gg, want_g) < 1e-4
        outs.append(gg)
    assert torch.equal(outs[0], outs[1])
    # frozen prompt (g NULL): the rows are zeroed all the same; vision placement (the last n rows of each sequence)
    dx = dx0.clone()
    LB.check(lib.clipfs_prompt_harvest(dx.data_ptr(), None, offp, batch, seq, first, n, width, None, st), "harvest")
    torch.cuda.synchronize()
    assert torch.equal(dx, want_dx)
    if not packed:
        x = torch.zeros(batch * seq, width, device=dev)
        LB.check(lib.clipfs_prompt_put(prompt.data_ptr(), x.data_ptr(), None, batch, seq, seq - n, n, width, st), "put")
        torch.cuda.synchronize()
        assert torch.equal(x.view(batch, seq, width)[:, seq - n:], prompt.expand(batch, n, width))
        assert not x.view(batch, seq, width)[:, :seq - n].any()


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [3, 6])
def test_features_and_gradients_match_fp64(dev, depth):
    """LoRA, ctx, VPT and every deep prompt of both towers; depth 6 puts a prompt on the last block (its compact part)."""
    s = _make(dev, depth)
    s.model.eval()
    logits, _ = _step(s)
    loss, wl, tl, vl, deep, octx, ovpt = _oracle(s)
    assert _err(logits, wl) < 1e-3
    assert abs(s.loss - loss.item()) < 1e-4
    pairs = []
    for i, layer in enumerate(s.layers):
        ref = (tl if i < 6 else vl)[i % 6]
        slot = dict((id(prm), g) for prm, g in layer.trainable_pairs())
        for pr in "qkv":
            m = getattr(layer, NAMES[pr])
            pairs += [(slot[id(m.w_lora_A)], ref[NAMES[pr]]["w_lora_A"].grad),
                      (slot[id(m.w_lora_B)], ref[NAMES[pr]]["w_lora_B"].grad)]
    pairs += [(s.ctx.grad_slot, octx.grad), (s.model.visual.VPT.grad_slot, ovpt.grad)]
    got = _deep(s.model)
    assert sorted(got["text"]) == sorted(got["vision"]) == list(range(1, depth))
    for tw in ("text", "vision"):
        for i, p in got[tw].items():
            pairs.append((p.grad_slot, deep[tw][i].grad))
    for g, w in pairs:
        assert w.abs().max().item() > 0
        assert _err(g, w) < 1e-4 * max(w.abs().max().item(), 1e-3), f"grad err {_err(g, w):.3e}"


# 3 ---------------------------------------------------------------------------------------------------------------
def _text_modes(s, lo):
    """(pack_mode, pack_fwd_mode) of the text tower for this model's caption table and floor ``lo``."""
    eng = s.model.engine
    ids = s.cap.contiguous()
    _, R = eng._pack_plan(ids)
    desc = eng.txt.descriptor(True, 1, ids.shape[1], 0, lo)
    return eng.txt.pack_modes(desc, ids.shape[0], R)


def test_paths_agree_with_dropout(dev):
    """pack_text_forward / pack_text_backward / sparse_backward on vs off, LoRA dropout 0.25.  The live-row forward is
    bitwise the dense one; the live-row backward gives the same logits and gradients up to summation order; the dense
    last block (sparse_backward off) sums its products in another order than the one-row-per-sequence products, which
    run split-K at 403 rows (clipfs.h, clipfs_gemm_splits), so logits and gradients agree up to summation order.  403
    captions x 77 tokens (bench.py's table size): the live-row forward and backward both run, so the prompt put of the
    packed forward and the harvest over its packed saved records are what the A legs check."""
    s = _make(dev, 3, p=0.25, Cn=403, context_length=77)
    s.model.train()
    ref_l, ref_g = _step(s)
    assert s.tr.last_plan == {"text": 0, "vision": 0}
    assert _text_modes(s, 0) == (True, True)
    assert _step(s)[1].equal(ref_g)  # reproducible
    scale = ref_g.abs().max().item()
    for flag, same_logits, exact in (("pack_text_forward", True, True), ("pack_text_backward", True, False),
                                     ("sparse_backward", False, False)):
        lg, gr = _step(s, **{flag: False})
        assert torch.equal(lg, ref_l) if same_logits else _err(lg, ref_l) < 1e-4, flag
        if exact:
            assert torch.equal(gr, ref_g), flag
        else:
            assert (gr - ref_g).abs().max().item() < 1e-5 * scale, flag


def test_prune_moves_the_floor_on_the_live_rows(dev):
    """prune_backward on vs off where the text floor moves (no ctx; the adapters of text blocks 0 and 1 frozen, so block
    1 trains its prompt only): floor 1 vs 0, on the live-row forward and backward, LoRA dropout 0.25.  Logits and
    gradients bitwise."""
    s = _make(dev, 3, p=0.25, Cn=403, context_length=77)
    for layer in s.layers[:2]:  # apply_lora order: text blocks first
        for prm, _ in layer.trainable_pairs():
            prm.requires_grad_(False)
    s.ctx = None
    s.model.train()
    ref_l, ref_g = _step(s)
    assert s.tr.last_plan == {"text": 1, "vision": 0}
    assert _text_modes(s, 1) == (True, True)
    lg, gr = _step(s, prune_backward=False)
    assert s.tr.last_plan == {"text": 0, "vision": 0}
    assert torch.equal(lg, ref_l) and torch.equal(gr, ref_g)
    assert s.model.transformer.resblocks[1].VPT_shallow.grad_slot.abs().max().item() > 0


# 4 ---------------------------------------------------------------------------------------------------------------
def test_floor_is_the_lowest_prompt_block(dev):
    """Frozen adapters, no ctx: the text tower's floor is its lowest prompt block, whose input gradient is formed (and
    harvested) although nothing below it needs one.  (The trainable VPT keeps the image tower's floor at 0.)"""
    s = _make(dev, 3)
    for layer in s.layers:
        for prm, _ in layer.trainable_pairs():
            prm.requires_grad_(False)
    s.ctx = None
    s.model.eval()
    _, g_pruned = _step(s)
    assert s.tr.last_plan == {"text": 1, "vision": 0}
    assert s.tr.flat.numel == 4 * 192 + 2 * 4 * (128 + 192)  # the VPT and the four deep prompts
    _, g_full = _step(s, prune_backward=False)
    assert s.tr.last_plan == {"text": 0, "vision": 0}
    assert torch.equal(g_pruned, g_full)
    assert g_pruned.abs().max().item() > 0


# 5 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,tol_logits,tol_grad", [("bf16x3", 1e-3, 1e-2), ("fp16", 2e-2, 1e-1)])
def test_other_precisions(dev, precision, tol_logits, tol_grad):
    s = _make(dev, 3)
    s.model.eval()
    ref_l, ref_g = _step(s)
    lg, gr = _step(s, precision=precision)
    assert _err(lg, ref_l) < tol_logits
    off = s.tr.flat.numel - sum(p.numel() for p in s.tr.flat.deep_prompts)  # the deep prompts' slice (no biases here)
    assert (gr[off:] - ref_g[off:]).abs().max().item() < tol_grad * ref_g[off:].abs().max().item()
    assert (gr - ref_g).abs().max().item() < tol_grad * ref_g.abs().max().item()


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "fp16"])
def test_replaced_rows_carry_no_gradient(dev, precision):
    """Every caption ends at or before row 4 (EOT <= language_ctx), so a prompted block replaces every row from 1 up to
    the EOT and the caption's feature depends on the block below through row 0 only.  Under the causal mask the rows
    1 ... 4 below block 2 then carry exactly zero gradient, in every precision: block 1's prompt and the ctx rows of the
    tower input get none, while block 2's prompt does.  Nonzero there would be gradient leaking through the replaced
    rows -- in the fp16 storage mode through the f16 image of dx the next block's GEMMs read, which the harvest must
    zero too (a leak below block 2 lands in block 1's prompt, one below block 1 in the ctx)."""
    s = _make(dev, 3, Cn=9, min_len=1, max_len=3)
    assert int(s.cap.argmax(dim=-1).max()) <= 4
    s.model.eval()
    _step(s, precision=precision)
    blocks = s.model.transformer.resblocks
    assert blocks[2].VPT_shallow.grad_slot.abs().max().item() > 0  # what would leak
    assert blocks[1].VPT_shallow.grad_slot.abs().max().item() == 0.0
    assert s.ctx.grad_slot.abs().max().item() == 0.0
    text_lora0 = [g for _, g in s.layers[0].trainable_pairs()]  # block 0 still trains (through row 0)
    assert max(g.abs().max().item() for g in text_lora0) > 0


# 6 ---------------------------------------------------------------------------------------------------------------
def test_lora_trainer_moves_deep_prompts(dev):
    s = _make(dev, 3)
    s.model.train()
    tr = s.L.LoRATrainer(s.model, prompt_ctx=s.ctx, lr=1e-3)
    before = {(tw, i): p.detach().clone() for tw, d in _deep(s.model).items() for i, p in d.items()}
    sd_before = {k for k in s.model.state_dict() if k.endswith("VPT_shallow")}
    for _ in range(3):
        tr.step(s.img, s.cap, s.tgt)
    torch.cuda.synchronize()
    after = _deep(s.model)
    for (tw, i), p0 in before.items():
        assert not torch.equal(after[tw][i].detach(), p0), (tw, i)
    # the trained values are what state_dict returns
    sd = s.model.state_dict()
    assert sd_before == {"transformer.resblocks.1.VPT_shallow", "transformer.resblocks.2.VPT_shallow",
                         "visual.transformer.resblocks.1.VPT_shallow", "visual.transformer.resblocks.2.VPT_shallow"}
    assert torch.equal(sd["visual.transformer.resblocks.2.VPT_shallow"], after["vision"][2].detach())


def test_stage2_trainer_moves_deep_prompts(dev):
    import slow_pace as S
    s = _make(dev, 3)
    for layer in s.layers:  # stage 2: LoRA applied but frozen
        for prm, _ in layer.trainable_pairs():
            prm.requires_grad_(False)
    for p in _deep(s.model)["text"].values():  # the stage-2 rule turns them on again
        p.requires_grad_(False)
    s.model.train()
    d, C = s.cfg.embed_dim, s.cap.shape[0]
    g = torch.Generator().manual_seed(1)
    unit = lambda t: t / t.norm(dim=-1, keepdim=True)
    zs_img = unit(torch.randn(s.img.shape[0], d, generator=g))
    zs_txt = unit(torch.randn(C, d, generator=g))
    learner = S.VLPromptLearner.__new__(S.VLPromptLearner)
    torch.nn.Module.__init__(learner)
    learner.ctx = torch.nn.Parameter(s.ctx.detach().clone())
    learner.tokenized_prompts, learner.n_ctx, learner.n_cls = s.cap, 4, C
    learner._model = [s.model]
    head = S.Channel_LP(d, C, device=dev)
    with torch.no_grad():
        head.fc.weight.copy_(zs_txt)
    tr = S.Stage2Trainer(s.model, learner, head, zs_img, zs_txt, lr=1e-3, total_epoch=20)
    before = {(tw, i): p.detach().clone() for tw, dd in _deep(s.model).items() for i, p in dd.items()}
    assert all(p.requires_grad for dd in _deep(s.model).values() for p in dd.values())
    for _ in range(3):
        tr.step(s.img, s.tgt, torch.arange(s.img.shape[0]))
    torch.cuda.synchronize()
    after = _deep(s.model)
    for (tw, i), p0 in before.items():
        assert not torch.equal(after[tw][i].detach(), p0), (tw, i)


# 7 ---------------------------------------------------------------------------------------------------------------
def test_depth_one_is_todays_model(dev):
    a = _make(dev, 1)
    b = _make(dev, 1, deep=False)
    assert not _deep(a.model)["text"] and not _deep(a.model)["vision"]
    for s in (a, b):
        s.model.train()
    la, ga = _step(a)
    lb, gb = _step(b)
    assert torch.equal(la, lb) and torch.equal(ga, gb)
