"""CLIP ModifiedResNet (RN50 family) on the HIP engine: the three new kernels against fp64, image features against the
fp64 restatement of the tower (modified_resnet_ref.py), and the public paths that must not care where image features come
from -- clip_logits, LoRATrainer with text adapters, evaluate_lora, ood.score_views -- against the oracle with the fp64
image features fed in as constants.

Bounds (each the repository's existing one for the same kind of arithmetic): pools and token assembly 1e-6 of the largest
entry (test_moco_gpu: global pool); attention 2e-5 (test_kernels_gpu.test_attention, forward); image features 2e-4 of the
largest entry (test_moco_gpu: a 50-layer fp32 convolution stack); logits 1e-3 on 100 x cosine; loss 1e-4; adapter and
prompt gradients 1e-4 of the largest gradient entry (test_mlp_lora_gpu: trainer versus fp64)."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import modified_resnet_ref as R

pytestmark = pytest.mark.gpu

GEOS = R.geometries()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _err(a, b):
    return (a.detach().double().cpu() - b.detach().double().cpu()).abs().max().item()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,H,W,C,k", [(2, 9, 7, 16, 2), (1, 8, 8, 20, 2), (2, 6, 6, 64, 3)])
def test_avgpool_nhwc(dev, N, H, W, C, k):
    from clipfs import _lib
    lib = _lib.load()
    x = _randn(N, C, H, W, seed=1)
    ho, wo = H // k, W // k
    xh = x.permute(0, 2, 3, 1).contiguous()
    xh[:, ho * k:] = float("nan")                 # rows and columns past the last full window: never read
    xh[:, :, wo * k:] = float("nan")
    xd = xh.to(dev)
    rows, guard = N * ho * wo, 3
    y = torch.full((rows + guard, C), 7.0, device=dev)
    _lib.check(lib.clipfs_avgpool_nhwc(xd.data_ptr(), y.data_ptr(), N, H, W, C, k, _stream()))
    want = F.avg_pool2d(x.double(), k).permute(0, 2, 3, 1).reshape(rows, C)
    e, scale = _err(y[:rows], want), want.abs().max().item()
    print(f"avgpool {N}x{H}x{W}x{C} k{k}: err {e:.3e} of {scale:.3e}")
    assert torch.isfinite(y).all() and e < 1e-6 * scale
    assert (y[rows:] == 7.0).all(), "output guard rows were written"


@pytest.mark.parametrize("N,HW,C", [(3, 4, 512), (2, 9, 1024), (2, 49, 2048)])
def test_attnpool_tokens(dev, N, HW, C):
    from clipfs import _lib
    lib = _lib.load()
    x, pos = _randn(N, HW, C, seed=2), _randn(HW + 1, C, seed=3)
    xd, pd = x.to(dev), pos.to(dev)
    tok = torch.full((N * (HW + 1) + 2, C), 7.0, device=dev)
    _lib.check(lib.clipfs_attnpool_tokens(xd.data_ptr(), pd.data_ptr(), tok.data_ptr(), N, HW, C, _stream()))
    want = R.attnpool_tokens(x.double(), pos.double()).reshape(N * (HW + 1), C)
    e, scale = _err(tok[:-2], want), want.abs().max().item()
    print(f"attnpool_tokens {N}x{HW}x{C}: err {e:.3e} of {scale:.3e}")
    assert e < 1e-6 * scale and (tok[-2:] == 7.0).all()
    # the rows are copies plus pos: exact in fp32
    assert torch.equal(tok[:-2].reshape(N, HW + 1, C)[:, 1:].cpu(), x + pos[1:])


def _attend(dev, N, L, heads, kscale=1.0, seed=4):
    from clipfs import _lib
    lib = _lib.load()
    c = heads * 64
    q, kv = _randn(N, c, seed=seed), _randn(N * L, 2 * c, seed=seed + 1)
    kv[:, :c] *= kscale
    qd, kvd = q.to(dev), kv.to(dev)
    out = torch.full((N + 1, c), 7.0, device=dev)
    _lib.check(lib.clipfs_attnpool_attend(qd.data_ptr(), kvd.data_ptr(), out.data_ptr(), N, L, heads, _stream()))
    kv64 = kv.double().reshape(N, L, 2, heads, 64)
    want = R.attention(q.double().reshape(N, heads, 64), kv64[:, :, 0], kv64[:, :, 1]).reshape(N, c)
    assert (out[N:] == 7.0).all()
    return out[:N], want


@pytest.mark.parametrize("N,L,heads", [(3, 5, 8), (2, 10, 16), (2, 50, 32), (1, 197, 64)])
def test_attnpool_attend(dev, N, L, heads):
    got, want = _attend(dev, N, L, heads)
    print(f"attnpool_attend N{N} L{L} heads{heads}: err {_err(got, want):.3e}")
    assert _err(got, want) < 2e-5


def test_attnpool_attend_subtracts_the_maximum(dev):
    """Keys scaled by 30: scores reach a hundred and more, exp() of which overflows fp32 unless the row maximum is taken
    off.  The rounding error of a score grows with the keys, and a softmax passes a score error on one for one, so the
    bound here is the unit-scale one times 30."""
    got, want = _attend(dev, 2, 50, 8, kscale=30.0, seed=9)
    assert torch.isfinite(got).all()
    print(f"attnpool_attend, keys x 30: err {_err(got, want):.3e}")
    assert _err(got, want) < 30 * 2e-5


# ---------------------------------------------------------------------------------------------------------------------
# image features
# ---------------------------------------------------------------------------------------------------------------------

_MODELS = {}


def _model(dev, name):
    """(geometry, fp32 state dict, model on the device), built once per geometry; read-only for the tests that share it."""
    if name not in _MODELS:
        from jclip.model import build_model
        geo = GEOS[name]
        sd = R.synth_sd(geo)
        _MODELS[name] = (geo, sd, build_model(sd, device=dev))
    return _MODELS[name]


_FEATS = {}


def _ref_features(name, sd, images):
    """fp64 image features of ``images`` (computed once per (geometry, batch) and shared)."""
    key = (name, tuple(images.shape), float(images.flatten()[0]))
    if key not in _FEATS:
        _FEATS[key] = R.image_features(R.to64(sd), images.double())
    return _FEATS[key]


@pytest.mark.parametrize("name,B", [("RN_TINY", 3), ("RN_SMALL", 2)])
def test_image_features(dev, name, B):
    from clipfs import synth
    geo, sd, model = _model(dev, name)
    img = synth.synth_images(B, geo.resolution, seed=3)
    got = model.encode_image(img.to(dev))
    want = _ref_features(name, sd, img)
    assert got.shape == (B, geo.embed) and not got.requires_grad
    e, scale = _err(got, want), want.abs().max().item()
    print(f"{name} image features: err {e:.3e} of {scale:.3e} ({e / scale:.2e} relative)")
    assert e < 2e-4 * scale
    # determinism: every summation order is fixed
    assert torch.equal(model.encode_image(img.to(dev)), got)
    # the engine's surface with such a tower
    eng = model.engine
    assert eng.image_plan() is None and not hasattr(eng, "vis") and not hasattr(eng, "vproj_t")
    feat, ctx = eng.vit_forward(img.to(dev), True, 1)
    assert ctx is None and torch.equal(feat, got)
    with pytest.raises(ValueError, match="expected images"):
        eng.vit_forward(img[:, :, :32, :32].contiguous().to(dev), False)
    eng.precision = "bf16x3"      # the text tower's setting; the image tower stays fp32
    try:
        assert eng.precision == "bf16x3" and torch.equal(model.encode_image(img.to(dev)), got)
    finally:
        eng.precision = "fp32"


def test_image_features_rn50_geometry(dev):
    """RN50 itself: layers (3, 4, 6, 3), width 64, 224 px, 32 heads over 50 tokens (synthetic weights)."""
    from clipfs import resnet, synth
    sd = resnet.synth_clip_resnet_state_dict((3, 4, 6, 3), 64, 224, 1024, seed=7)
    run = resnet.ClipResNet(sd, dev)
    assert run.layers == (3, 4, 6, 3) and run.heads == 32 and run.input_resolution == 224 and run.output_dim == 1024
    img = synth.synth_images(2, 224, seed=3)
    got = run(img.to(dev))
    want = R.image_features(R.to64(sd), img.double())
    e, scale = _err(got, want), want.abs().max().item()
    print(f"RN50 geometry image features: err {e:.3e} of {scale:.3e} ({e / scale:.2e} relative)")
    assert got.shape == (2, 1024) and e < 2e-4 * scale
    assert torch.equal(run(img.to(dev)), got)


def test_clip_logits(dev):
    from clipfs import synth
    from oracle import clip_oracle as O
    geo, sd, model = _model(dev, "RN_TINY")
    img = synth.synth_images(3, geo.resolution, seed=3)
    cap = synth.synth_captions(5, geo.text.context_length, geo.text.vocab_size, seed=4, max_len=12)
    li, lt = model(img.to(dev), cap.to(dev))
    sd64 = R.to64(sd)
    fi = O.l2_normalize(_ref_features("RN_TINY", sd, img))
    ft = O.l2_normalize(O.encode_text(sd64, cap))
    want = sd64["logit_scale"].exp() * fi @ ft.t()
    print(f"clip_logits: err {_err(li, want):.3e}")
    assert _err(li, want) < 1e-3 and torch.equal(lt, li.t())


# ---------------------------------------------------------------------------------------------------------------------
# training the text side against a frozen ModifiedResNet
# ---------------------------------------------------------------------------------------------------------------------

PARAMS = ("q", "k", "v")
NAMES = {"q": "q_proj", "k": "k_proj", "v": "v_proj"}


def _make_trainable(dev, p, with_ctx, r=4):
    import lora_train_vlp as L
    from jclip.model import build_model
    geo = GEOS["RN_TINY"]
    sd = R.synth_sd(geo)
    model = build_model(sd, device=dev)
    args = types.SimpleNamespace(encoder="text", position="all", backbone="RN50", params=list(PARAMS), r=r, alpha=1,
                                 dropout_rate=p)
    saved = L.INDEX_POSITIONS_TEXT["all"]
    L.INDEX_POSITIONS_TEXT["all"] = list(range(geo.text.transformer_layers))
    try:
        layers = L.apply_lora(args, model)
    finally:
        L.INDEX_POSITIONS_TEXT["all"] = saved
    assert len(layers) == geo.text.transformer_layers
    rng = np.random.RandomState(5)
    weights = []
    with torch.no_grad():
        for layer in layers:
            w = {}
            for tok in PARAMS:
                m = getattr(layer, NAMES[tok])
                fout, fin = m.w_lora_B.shape[0], m.w_lora_A.shape[1]
                a = rng.uniform(-1, 1, size=(r, fin)).astype(np.float32) / np.float32(np.sqrt(fin))
                b = (rng.standard_normal((fout, r)) * 0.05).astype(np.float32)
                m.w_lora_A.copy_(torch.from_numpy(a))
                m.w_lora_B.copy_(torch.from_numpy(b))
                w[NAMES[tok]] = {"w_lora_A": a, "w_lora_B": b}
            weights.append(w)
    L.mark_only_lora_as_trainable(model, "none")
    ctx = torch.nn.Parameter(sd["token_embedding.weight"][[5, 6, 7, 8]].clone().to(dev)) if with_ctx else None
    return types.SimpleNamespace(L=L, geo=geo, sd=sd, model=model, layers=layers, weights=weights, ctx=ctx, p=p, r=r)


def _batch(geo, B=6, Cn=9):
    from clipfs import synth
    return (synth.synth_images(B, geo.resolution, seed=3),
            synth.synth_captions(Cn, geo.text.context_length, geo.text.vocab_size, seed=4, max_len=12),
            synth.synth_labels(B, Cn, seed=2))


def _oracle_step(S, img, cap, tgt, seed):
    """Loss and logits of the step in fp64 autograd: the oracle's text tower with the adapters (and the dropout masks of
    ``seed``), the helper's image features as constants.  Returns (loss, logits, adapter leaves per block, ctx leaf)."""
    from oracle import clip_oracle as O
    cfg = S.geo.text
    sd64 = R.to64(S.sd)
    tl = {b: {k: {n: torch.from_numpy(v).double().requires_grad_(True) for n, v in ab.items()} for k, ab in w.items()}
          for b, w in enumerate(S.weights)}
    octx = S.ctx.detach().double().cpu().requires_grad_(True) if S.ctx is not None else None
    Cn = cap.shape[0]
    drops = None
    if S.p > 0:  # element (global token row, column) of stream 4 * block + projection (clipfs/engine.py)
        drops = {}
        for l in tl:
            d = {}
            for s, tok in enumerate(PARAMS):
                keep = O.dropout_keep_mask(seed, 4 * l + s, Cn * cfg.context_length, cfg.transformer_width, S.p)
                d[NAMES[tok]] = (torch.from_numpy(keep).double() / (1 - S.p)).reshape(
                    Cn, cfg.context_length, cfg.transformer_width).permute(1, 0, 2)
            drops[l] = d
    scaling = O.lora_scaling(1, S.r)
    if octx is None:
        emb = O.encode_text(sd64, cap, tl, scaling, drops=drops)
    else:
        emb = O.encode_text(sd64, cap, tl, scaling, embeds=O.build_prompts(octx, sd64["token_embedding.weight"], cap),
                            drops=drops)
    txt = O.class_text_features(emb, list(range(Cn)), Cn)
    fi = _ref_features("RN_TINY", S.sd, img).detach()
    logits = O.train_logits(fi, txt)
    return O.jt_cross_entropy(logits, tgt), logits, tl, octx


@pytest.mark.parametrize("with_ctx", [False, True], ids=["plain", "ctx"])
@pytest.mark.parametrize("p", [0.0, 0.25])
def test_lora_trainer_step_against_fp64(dev, p, with_ctx):
    from clipfs.engine import _mix_seed
    S = _make_trainable(dev, p, with_ctx)
    img, cap, tgt = _batch(S.geo)
    B = img.shape[0]
    S.model.train()
    tr = S.L.LoRATrainer(S.model, prompt_ctx=S.ctx)
    tr.flat.zero_grad()
    loss_sum, correct, logits = tr.forward_backward(img.to(dev), cap.to(dev), tgt.to(dev))
    assert tr.last_plan["vision"] is None and tr.last_plan["text"] == 0
    seed = _mix_seed(S.model.engine.seed_base, S.model.engine.step)
    loss, wlogits, tl, octx = _oracle_step(S, img, cap, tgt, seed)
    loss.backward()
    print(f"logits err {_err(logits, wlogits):.3e}, loss err {abs(loss_sum.item() / B - loss.item()):.3e}")
    assert _err(logits, wlogits) < 1e-3
    assert abs(loss_sum.item() / B - loss.item()) < 1e-4
    assert correct.item() == int((wlogits.argmax(1) == tgt).sum())
    leaves = [(S.layers[b], NAMES[tok], nm, tl[b][NAMES[tok]][nm]) for b in tl for tok in PARAMS
              for nm in ("w_lora_A", "w_lora_B")]
    gmax = max(t.grad.abs().max().item() for *_, t in leaves)
    worst = 0.0
    for layer, proj, nm, t in leaves:
        slot = dict((id(q), g) for q, g in layer.trainable_pairs())[id(getattr(getattr(layer, proj), nm))]
        assert t.grad.abs().max().item() > 0
        worst = max(worst, _err(slot, t.grad))
    print(f"adapter gradients: worst err {worst:.3e}, largest entry {gmax:.3e}")
    assert worst < 1e-4 * max(gmax, 1e-3)
    if with_ctx:
        assert _err(S.ctx.grad_slot, octx.grad) < 1e-4 * max(octx.grad.abs().max().item(), 1e-3)


def _steps(tr, batch, n):
    return [tr.step(*batch)[0].clone() for _ in range(n)]


def test_lora_trainer_three_steps_and_resume(dev):
    kw = dict(lr=1e-3, max_grad_norm=1.0, ema_decay=0.99, loss_scale="dynamic")
    a = _make_trainable(dev, 0.25, True)
    batch = tuple(t.to(dev) for t in _batch(a.geo))
    a.model.train()
    ta = a.L.LoRATrainer(a.model, prompt_ctx=a.ctx, **kw)
    p0 = ta.flat.params.clone()
    losses_a = _steps(ta, batch, 3)
    assert all(torch.isfinite(x).all() for x in losses_a) and not torch.equal(ta.flat.params, p0)
    assert ta.last_plan["vision"] is None and (ta.t, ta.skipped_steps) == (3, 0)
    b = _make_trainable(dev, 0.25, True)
    b.model.train()
    tb = b.L.LoRATrainer(b.model, prompt_ctx=b.ctx, **kw)
    losses_b = _steps(tb, batch, 1)
    sd = tb.state_dict()
    c = _make_trainable(dev, 0.25, True)   # a freshly built model and trainer
    c.model.train()
    tc = c.L.LoRATrainer(c.model, prompt_ctx=c.ctx, **kw)
    tc.load_state_dict(sd)
    losses_b += _steps(tc, batch, 2)
    for x, y in zip(losses_a, losses_b):
        assert torch.equal(x, y)
    for x, y in ((ta.flat.params, tc.flat.params), (ta.flat.m, tc.flat.m), (ta.flat.v, tc.flat.v),
                 (ta.ema_shadow, tc.ema_shadow)):
        assert torch.equal(x, y)


# ---------------------------------------------------------------------------------------------------------------------
# evaluation paths
# ---------------------------------------------------------------------------------------------------------------------

def test_evaluate_lora_and_score_views(dev):
    import lora_train_vlp as L
    import ood
    from clipfs import synth
    from oracle import clip_oracle as O
    geo, sd, model = _model(dev, "RN_TINY")
    n_img, V, Cn = 4, 5, 6
    res = geo.resolution
    # images: a base image per class, the first n_img of them with V - 1 noisy copies behind the clean centre view
    base = synth.synth_images(Cn, res, seed=21)
    views = base[:n_img, None] + 0.5 * synth.synth_images(n_img * V, res, seed=22).reshape(n_img, V, 3, res, res)
    views[:, 0] = base[:n_img]
    sd64 = R.to64(sd)
    # classes: what tells the base images' features apart (random weights put most of every feature into one common
    # direction; captions would send every image to the same class, which checks little)
    proto = O.l2_normalize(R.image_features(sd64, base.double()))
    common = O.l2_normalize(proto.mean(dim=0, keepdim=True))
    text = O.l2_normalize(proto - (proto @ common.t()) * common)                     # [C, d] unit rows
    feats = O.l2_normalize(R.image_features(sd64, views.reshape(n_img * V, 3, res, res).double())).reshape(n_img, V, -1)
    want_mta = torch.cat([O.solve_mta(feats[i], text.t()) for i in range(n_img)])    # [n_img, C]
    want_top1 = want_mta.argmax(1)
    base_l, ens_l = feats[:, 0] @ text.t() * 100, feats.mean(dim=1) @ text.t() * 100
    for x in (want_mta, base_l, ens_l):  # 100 x cosine is good to 1e-3 here: the oracle's decisions must not hang on less
        top2 = x.topk(2, dim=1).values
        assert ((top2[:, 0] - top2[:, 1]) > 1e-2).all(), "a near tie in the oracle's scores: pick other seeds"
    assert len(set(want_top1.tolist())) == n_img, "every image in the same class: the check would be weak"
    text_dev = text.float().to(dev)
    top5, is_base, logits = ood.score_views(model, views.to(dev), text_dev)
    print(f"score_views: MTA logits err {_err(logits, want_mta):.3e}")
    assert torch.equal(top5[:, 0].long().cpu(), want_top1) and is_base.all()
    # tta.evaluate_views: the same tower as both the adapted and the zero-shot model, one classifier for all three roles
    import tta
    fused = tta.evaluate_views(model, model, views.to(dev), text_dev, text_dev, text_dev)
    assert torch.equal(fused["top5"][:, 0].long().cpu(), want_top1) and torch.equal(fused["cos4"].argmax(1).cpu(), want_top1)
    # evaluate_lora: accuracies of the MTA, the centre view and the view mean against labels the oracle half agrees with
    target = want_top1.clone()
    target[1] = (target[1] + 1) % Cn
    loader = [(views[i:i + 2, 0], views[i:i + 2, 1:], target[i:i + 2], None) for i in (0, 2)]
    acc = L.evaluate_lora(None, model, loader, textual_features=text_dev.t().contiguous())
    want = tuple(100.0 * float((x.argmax(1) == target).sum()) / n_img for x in (want_mta, base_l, ens_l))
    assert acc == want and acc[0] == 75.0


# ---------------------------------------------------------------------------------------------------------------------
# stage 2: the unfused trainer only needs the tower's features; the fused step refuses the backbone by name
# ---------------------------------------------------------------------------------------------------------------------

def test_stage2_unfused_step_and_fused_refusal(dev):
    """One unfused Stage2Trainer step (prompt ctx + Channel_LP head; there is no VPT) against the oracle's stage-2 loss with
    the fp64 image features as constants: the bounds of test_stage2.py's step test (loss 5e-5 relative, gradients 5e-4 of
    the largest entry)."""
    import slow_pace as S
    from clipfs import synth
    from jclip.model import build_model
    from oracle import clip_oracle as O
    geo = GEOS["RN_TINY"]
    cfg = geo.text
    sd = R.synth_sd(geo)
    model = build_model(sd, device=dev)  # its own model: the trainer flags parameters
    model.eval()
    B, C, d = 6, 5, geo.embed
    g = torch.Generator().manual_seed(1)
    unit = lambda t: t / t.norm(dim=-1, keepdim=True)
    images = synth.synth_images(B, geo.resolution, seed=3)
    target = synth.synth_labels(B, C, seed=2)
    zs_img = unit(torch.randn(B, d, generator=g, dtype=torch.float64))
    zs_txt = unit(torch.randn(C, d, generator=g, dtype=torch.float64))
    ids = synth.synth_captions(C, cfg.context_length, cfg.vocab_size, seed=4, max_len=12)
    learner = S.VLPromptLearner.__new__(S.VLPromptLearner)
    torch.nn.Module.__init__(learner)
    learner.ctx = torch.nn.Parameter(model.token_embedding.weight.data[ids[0, 1:5].to(dev)].clone())
    learner.tokenized_prompts, learner.n_ctx, learner.n_cls = ids.to(dev), 4, C
    learner._model = [model]
    head = S.Channel_LP(d, C, device=dev)
    with torch.no_grad():
        head.fc.weight.copy_(zs_txt.float())
        head.scale1.copy_(1 + 0.1 * torch.randn(d, generator=g))
    with pytest.raises(ValueError, match="ModifiedResNet.*fused=False"):
        S.Stage2Trainer(model, learner, head, zs_img, zs_txt, fused=True)
    tr = S.Stage2Trainer(model, learner, head, zs_img, zs_txt, lr=1e-3, total_epoch=20)
    assert len(tr.params) == 1 + len(list(head.parameters()))
    p0 = [p.detach().clone() for p in tr.params]
    loss, _, _ = tr.step(images.to(dev), target.to(dev), torch.arange(B))
    sd64 = R.to64(sd)
    ctx64 = p0[0].double().cpu().requires_grad_()
    emb = sd64["token_embedding.weight"][ids]
    prompts = torch.cat([emb[:, :1], ctx64.unsqueeze(0).expand(C, -1, -1), emb[:, 5:]], dim=1)   # slow_pace.py:185-199
    txt = O.encode_text(sd64, ids, embeds=prompts)
    img = R.image_features(sd64, images.double()).detach()
    lp64 = [t.double().cpu().requires_grad_() for t in p0[1:]]
    ref, _, _ = O.stage2_loss(img, txt, target, zs_img, zs_txt, tuple(lp64), img, zs_txt)
    ref.backward()
    print(f"stage 2: loss {loss.item():.6f} vs {ref.item():.6f}")
    assert abs(loss.item() - ref.item()) < 5e-5 * abs(ref.item())
    for p, w in zip(tr.params, [ctx64.grad] + [t.grad for t in lp64]):
        assert _err(p.grad, w) <= 5e-4 * max(w.abs().max().item(), 1e-6)
