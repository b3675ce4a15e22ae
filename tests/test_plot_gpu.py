"""PLOT on the GPU (plot.py, clipfs.engine.encode_image_tokens) against the fp64 oracle: the local tokens of the SMALL
model (9 patches, LoRA adapters applied and frozen, built as test_tpt_gpu._build does), one PLOTTrainer step (loss, the
gradient of both ctx blocks, the AdamW update), the state dict round trip and the refusals.

Yardstick of the two parity tests: the SAME oracle pipeline evaluated in fp32 on the CPU against its fp64 evaluation, x 8,
with the floor 2^-24 max |ref|; nothing from the device enters it.  Each test prints measured / tol before it asserts.
Measured on one MI355X (error, the fp32 CPU evaluation's error, measured / tol): tokens 4.92e-6, 4.51e-6, 0.137; class
row 1.69e-6, 1.81e-6, 0.117, and bitwise encode_image's dense route; step loss 4.41e-7, 2.02e-7, 0.272; ctx gradient
1.14e-6 of a largest entry 0.694, 9.25e-7, 0.155 (the autograd form 9.54e-7, 0.129); ctx after AdamW 4.51e-9, 0.054 of
its bound."""
import types

import pytest
import torch

import ot_ref as R
from poison import same_bits
from test_tpt_gpu import _build, _oracle_text

pytestmark = pytest.mark.gpu
EPS32 = 2.0 ** -24
N_PROMPTS, LR, WD = 2, 5e-3, 0.01
_SHARED = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _tol(ref64, ref32, factor=8.0):
    e32 = float((ref32.double() - ref64).abs().max())
    return factor * max(e32, EPS32 * float(ref64.abs().max())), e32


def _model(dev):
    """The SMALL model with the fp64 and fp32 oracle pieces of both towers; built once, read-only."""
    if "m" not in _SHARED:
        from clipfs import synth
        m = _build(dev)
        lw = synth.synth_lora(m.cfg, 4, seed=5)
        conv = lambda d: {p: {k: torch.from_numpy(v).double() for k, v in ab.items()} for p, ab in d.items()}
        m.vl = {b: conv(lw[f"layer_{m.cfg.transformer_layers + b}"]) for b in range(m.cfg.vision_layers)}
        f32 = lambda layers: {b: {p: {k: v.float() for k, v in ab.items()} for p, ab in d.items()} for b, d in layers.items()}
        m.m32 = types.SimpleNamespace(O=m.O, ids=m.ids, sc=m.sc, sd64={k: v.float() for k, v in m.sd64.items()}, tl=f32(m.tl),
                                      vl=f32(m.vl))
        m.images = synth.synth_images(4, m.cfg.image_resolution, seed=3)
        _SHARED["m"] = m
    return _SHARED["m"]


def _oracle_tokens(m, images):
    """[B, L, e]: every row of the oracle's image tower through ln_post and proj, in the dtype of m's weights."""
    O, sd = m.O, m.sd64
    x = O.encode_image(sd, images.to(sd["visual.proj"].dtype), m.vl, m.sc, return_tokens=True)
    return O.jt_layer_norm(x, sd["visual.ln_post.weight"], sd["visual.ln_post.bias"]) @ sd["visual.proj"]


def test_tokens_match_the_oracle(dev):
    from clipfs import engine as E
    m = _model(dev)
    P = (m.cfg.image_resolution // m.cfg.vision_patch_size) ** 2
    assert P == 9
    tokens, cls = E.encode_image_tokens(m.model, m.images.to(dev), with_class=True)
    assert tuple(tokens.shape) == (4, P, m.cfg.embed_dim) and tuple(cls.shape) == (4, m.cfg.embed_dim)
    assert same_bits(tokens, m.model.encode_image_tokens(m.images.to(dev)))
    with torch.no_grad():
        ref64, ref32 = _oracle_tokens(m, m.images), _oracle_tokens(m.m32, m.images)
    tol_t, e_t = _tol(ref64[:, 1:1 + P], ref32[:, 1:1 + P])
    tol_c, e_c = _tol(ref64[:, 0], ref32[:, 0])
    err_t = float((tokens.double().cpu() - ref64[:, 1:1 + P]).abs().max())
    err_c = float((cls.double().cpu() - ref64[:, 0]).abs().max())
    # the class row against encode_image's dense route
    eng = m.model.engine
    eng.sparse_backward = False
    try:
        feat = m.model.encode_image(m.images.to(dev))
    finally:
        eng.sparse_backward = True
    err_f = float((cls.double().cpu() - feat.double().cpu()).abs().max())
    print(f"tokens: err {err_t:.2e} (fp32 on the CPU {e_t:.2e}), measured / tol {err_t / tol_t:.3f} | class row {err_c:.2e} "
          f"({e_c:.2e}), {err_c / tol_c:.3f} | class row against encode_image {err_f:.2e}, {err_f / tol_c:.3f}")
    assert err_t <= tol_t and err_c <= tol_c and err_f <= tol_c


def _plot(m, dev, seed=0):
    import plot
    learner = plot.PLOTPromptLearner.from_token_ids(m.ids, m.model, n_prompts=N_PROMPTS, n_ctx=4, seed=seed)
    return plot, learner, plot.PLOTClassifier(m.model, learner, eps=0.1, iters=100)


def _batch(m, dev, cl):
    if "batch" not in _SHARED:
        tokens = cl.tokens(m.images.to(dev))
        labels = torch.tensor([1, 4, 0, 2])
        _SHARED["batch"] = (tokens, labels)
    return _SHARED["batch"]


def _oracle_step(mo, ctx, tokens, labels, cl, dtype):
    """(loss, ctx gradient [N, n_ctx, d]) of the mean cross entropy through the oracle text tower and ot_ref in ``dtype``."""
    ctx = ctx.to(dtype).clone().requires_grad_(True)
    text = torch.stack([_oracle_text(mo, ctx[n]) for n in range(ctx.shape[0])], dim=1)  # [C, N, e]
    logits = R.forward(tokens, text, None, None, cl.eps, cl.iters, cl.scale, dtype)["logits"]
    loss = mo.O.jt_cross_entropy(logits, labels)
    loss.backward()
    return loss.detach(), ctx.grad


def test_one_step_matches_the_oracle(dev):
    m = _model(dev)
    plot, learner, cl = _plot(m, dev)
    tokens, labels = _batch(m, dev, cl)
    trainer = plot.PLOTTrainer(cl, lr=LR, weight_decay=WD)
    ctx0 = learner.ctx.detach().clone()
    assert learner.ctx.data_ptr() == trainer.params.data_ptr()  # the blocks are views of the flat buffer
    logits0 = cl.logits(tokens).detach()
    loss, correct = trainer.step(tokens, labels.to(dev))
    grad = trainer.ctx_grad.clone()
    l64, g64 = _oracle_step(m, ctx0.cpu(), tokens.cpu(), labels, cl, torch.float64)
    l32, g32 = _oracle_step(m.m32, ctx0.cpu(), tokens.cpu(), labels, cl, torch.float32)
    tol_l, e_l = _tol(l64, l32)
    tol_g, e_g = _tol(g64, g32)
    err_l = abs(float(loss.item()) - float(l64))
    err_g = float((grad.double().cpu() - g64).abs().max())
    print(f"PLOT step: loss {float(l64):.4f} err {err_l:.2e} (fp32 on the CPU {e_l:.2e}), measured / tol {err_l / tol_l:.3f} | "
          f"ctx grad err {err_g:.2e} of max {float(g64.abs().max()):.2e} ({e_g:.2e}), {err_g / tol_g:.3f}")
    assert float(g64[0].abs().max()) > 1e-4 and float(g64[1].abs().max()) > 1e-4  # both blocks carry gradient
    assert int(correct.item()) == int((logits0.argmax(1).cpu() == labels).sum())
    assert err_l <= tol_l and err_g <= tol_g
    # AdamW from zero moments, step 1, on the ENGINE's gradient.  fp32 costs a few roundings of each of the two terms
    # p (1 - lr wd) and lr m^ / (sqrt(v^) + eps), the second at most lr: 16 x 2^-24 (max |p| + lr)
    want, _, _ = m.O.jt_adamw_step(ctx0.double().cpu(), grad.double().cpu(), torch.zeros_like(g64), torch.zeros_like(g64), 1,
                                   lr=LR, weight_decay=WD)
    err_p = float((learner.ctx.detach().double().cpu() - want).abs().max())
    tol_p = 16 * EPS32 * (float(ctx0.abs().max()) + LR)
    print(f"PLOT step: ctx after AdamW err {err_p:.2e}, measured / tol {err_p / tol_p:.3f}")
    assert err_p <= tol_p and not same_bits(learner.ctx.detach(), ctx0)
    # the autograd form gives the step's gradient
    _, learner2, cl2 = _plot(m, dev)
    torch.nn.functional.cross_entropy(cl2.logits(tokens), labels.to(dev)).backward()
    err_a = float((learner2.ctx.grad.double().cpu() - g64).abs().max())
    print(f"PLOT autograd: ctx grad err {err_a:.2e}, measured / tol {err_a / tol_g:.3f}")
    assert err_a <= tol_g


def test_forward_on_images_is_logits_on_their_tokens(dev):
    m = _model(dev)
    plot, learner, cl = _plot(m, dev)
    tokens, labels = _batch(m, dev, cl)
    with torch.no_grad():
        assert same_bits(cl(m.images.to(dev)), cl.logits(tokens))
    acc = plot.evaluate_plot(cl, tokens, labels, batch=3)
    with torch.no_grad():
        assert acc == float((cl.logits(tokens).argmax(1).cpu() == labels).sum()) / 4


def test_state_dict_round_trip_is_bitwise(dev):
    m = _model(dev)
    plot, learner, cl = _plot(m, dev)
    tokens, labels = _batch(m, dev, cl)
    labels = labels.to(dev)
    a = plot.PLOTTrainer(cl, lr=LR, weight_decay=WD, T_max=10)
    a.step(tokens, labels)
    sd = a.state_dict()
    la, _ = a.step(tokens, labels)
    _, learner_b, cl_b = _plot(m, dev, seed=9)  # another initialisation: everything must come from the state
    b = plot.PLOTTrainer(cl_b, lr=1.0, weight_decay=0.5, T_max=10)
    b.load_state_dict(sd)
    lb, _ = b.step(tokens, labels)
    assert same_bits(la, lb) and same_bits(a.params, b.params) and same_bits(a.m, b.m) and same_bits(a.v, b.v)
    assert a.t == b.t == 2 and a.lr == b.lr
    for k, v in a.state_dict().items():
        w = b.state_dict()[k]
        assert same_bits(v, w) if torch.is_tensor(v) else v == w, k


def test_no_host_synchronisation_in_a_step(dev):
    m = _model(dev)
    plot, learner, cl = _plot(m, dev)
    tokens, labels = _batch(m, dev, cl)
    labels = labels.to(dev)
    trainer = plot.PLOTTrainer(cl, lr=LR, weight_decay=WD)
    trainer.step(tokens, labels)  # warm-up: the text tower's row plan of this prompt table, the workspaces
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, _ = trainer.step(tokens, labels)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(loss).all())


def test_refusals(dev):
    import modified_resnet_ref as RN
    import plot
    from clipfs import engine as E
    from clipfs import synth
    from jclip.model import build_model
    m = _model(dev)
    geo = RN.geometries()["RN_TINY"]
    rn = build_model(RN.synth_sd(geo), device=dev)
    with pytest.raises(ValueError, match="ModifiedResNet"):
        E.encode_image_tokens(rn, synth.synth_images(1, geo.resolution, seed=3).to(dev))
    ids = synth.synth_captions(3, geo.text.context_length, geo.text.vocab_size, seed=4, max_len=10)
    with pytest.raises(ValueError, match="ModifiedResNet"):
        plot.PLOTClassifier(rn, plot.PLOTPromptLearner.from_token_ids(ids, rn, n_prompts=2))
    _, learner, cl = _plot(m, dev)
    lora = [p for n, p in m.model.named_parameters() if "lora_" in n]
    try:
        for p in lora:
            p.requires_grad_(True)
        with pytest.raises(ValueError, match="trainable adapters"):
            plot.PLOTClassifier(m.model, learner)
        with pytest.raises(ValueError, match="trainable adapters"):
            plot.PLOTTrainer(cl)
    finally:
        for p in lora:
            p.requires_grad_(False)
    with pytest.raises(ValueError, match="n_prompts"):
        plot.PLOTPromptLearner.from_token_ids(m.ids, m.model, n_prompts=33)
