"""Test-time prompt tuning on the GPU: the objective kernel (clipfs_tpt_objective) against the fp64 reference of
tests/tpt_ref.py -- values, selection, ties, text / selection modes, determinism -- and the episodes of
tpt.TestTimePromptTuner against the fp64 oracle: ctx gradient, AdamW step, final logits, the shared first forward, what an
episode must leave untouched, host synchronisation, a ModifiedResNet tower, the fp16 storage mode and the refusals.

Every bound below is 4 x the worst error measured over this file's cases on one MI355X (DESIGN.md section 23 lists
measured value and bound); each test prints its figures before it asserts."""
import dataclasses
import types

import pytest
import torch

from tpt_ref import entropy_gap, tpt_inputs, tpt_ref

pytestmark = pytest.mark.gpu

S100 = 100.0
# kernel against fp64: the worst error over the cases of section 1 (section 2 reuses the bounds) was 9.20e-6 (loss, at
# (65, 1000, 600, 6)), 3.23e-5 (entropy, same case) and 2.88e-5 of the largest entry (dtext, at (5, 3, 64, 1))
LOSS_TOL = 3.7e-5    # |loss - ref|
ENT_TOL = 1.3e-4     # max |H - ref|
DT_TOL = 1.2e-4      # max |dtext - ref| / max |ref|
# episodes against the fp64 oracle (sections 5 and 7)
CTX_GRAD_TOL = 1.6e-5      # max |ctx_grad - oracle| / max |oracle|: measured 3.86e-6
EP_LOGIT_TOL = 1.2e-4      # max |logits - oracle's at the engine's tuned ctx|: measured 2.80e-5
RN_CTX_GRAD_TOL = 9.3e-6   # the ModifiedResNet model: measured 2.31e-6
FP16_CTX_GRAD_TOL = 1.1e-2  # fp16 storage mode with loss_scale 4096 against the fp32 episode: measured 2.72e-3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ shared references
_REF = {}


def _ref(V, C, d, K, seed):
    """(F, T, loss, dT, H, selected) of one image; computed once, shared, never written."""
    key = (V, C, d, K, seed)
    if key not in _REF:
        F, T = tpt_inputs(V, C, d, seed)
        _REF[key] = (F, T) + tpt_ref(F, T, K, S100)
    return _REF[key]


def _batch(dev, V, C, d, K, seeds):
    refs = [_ref(V, C, d, K, s) for s in seeds]
    feats = torch.stack([r[0] for r in refs]).to(dev)
    text = refs[0][1].to(dev) if len(seeds) == 1 else torch.stack([r[1] for r in refs]).to(dev)  # shared | one per image
    return refs, feats, text


def _errors(refs, loss, dtext, entropy):
    el = max(abs(loss[i].item() - r[2].item()) for i, r in enumerate(refs))
    eh = max((entropy[i].double().cpu() - r[4]).abs().max().item() for i, r in enumerate(refs))
    ed = max((dtext[i].double().cpu() - r[3]).abs().max().item() / r[3].abs().max().item() for i, r in enumerate(refs))
    return el, eh, ed


# ------------------------------------------------------------------------------------- 1. the kernel against tpt_ref
# (V, C, d, K): the bench shape; a tile's corner; V, C, d past a tile and a 64-feature step, C past the reduction's 1024
# threads' stride; one selected view and fewer views than a wave; odd everything; K = V; d at its limit over 4 steps
CASES = [(64, 403, 512, 6), (8, 6, 64, 2), (65, 1000, 600, 6), (5, 3, 64, 1), (33, 130, 192, 3), (64, 403, 512, 64),
         (128, 37, 1024, 12)]


def _seeds(case, n_img):
    if case == (128, 37, 1024, 12):  # only seeds 2 and 3 leave an entropy gap of 5e-3 at K here
        return (2,) if n_img == 1 else (3, 2, 3)
    return (0,) if n_img == 1 else (1, 2, 3)


@pytest.mark.parametrize("n_img", [1, 3])
@pytest.mark.parametrize("case", CASES, ids=["x".join(map(str, c)) for c in CASES])
def test_objective_matches_reference(dev, case, n_img):
    from clipfs import ops
    V, C, d, K = case
    refs, feats, text = _batch(dev, V, C, d, K, _seeds(case, n_img))
    for r in refs:  # on the REFERENCE: the selection is well separated, so the set must be the reference's
        assert entropy_gap(r[4], K) >= 5e-3
    loss, sel, dtext, ent = ops.tpt_objective(feats, text, K, S100, want_entropy=True)
    assert sel.dtype == torch.int32 and tuple(sel.shape) == (n_img, K) and tuple(dtext.shape) == (n_img, C, d)
    for i, r in enumerate(refs):
        assert sel[i].tolist() == r[5].tolist()
    el, eh, ed = _errors(refs, loss, dtext, ent)
    print(f"tpt {case} n_img {n_img}: loss err {el:.2e}, entropy err {eh:.2e}, dtext err {ed:.2e} of the largest entry")
    assert el <= LOSS_TOL and eh <= ENT_TOL and ed <= DT_TOL


# ------------------------------------------------------------------------------------------------------- 2. large V
@pytest.mark.parametrize("case", [(513, 12, 128, 51), (1024, 37, 64, 102)], ids=["513", "1024"])
def test_objective_large_v(dev, case):
    """Entropy gaps at K are below the kernel's entropy error here: any set that differs from the reference's only in
    views within ENT_TOL of the K-th entropy is accepted, and loss / gradient are compared for the kernel's set."""
    from clipfs import ops
    V, C, d, K = case
    F, T, _, _, H, _ = _ref(V, C, d, K, 0)
    loss, sel, dtext, ent = ops.tpt_objective(F.to(dev)[None], T.to(dev), K, S100, want_entropy=True)
    got = sel[0].long().cpu()
    assert got.tolist() == sorted(set(got.tolist())) and got.numel() == K and 0 <= int(got[0]) and int(got[-1]) < V
    hk = torch.sort(H).values[K - 1].item()
    inside = torch.zeros(V, dtype=torch.bool)
    inside[got] = True
    assert (H[inside] <= hk + ENT_TOL).all() and (H[~inside] >= hk - ENT_TOL).all()
    rl, rd, _, _ = tpt_ref(F, T, K, S100, selected=got)
    el = abs(loss.item() - rl.item())
    eh = (ent[0].double().cpu() - H).abs().max().item()
    ed = (dtext[0].double().cpu() - rd).abs().max().item() / rd.abs().max().item()
    print(f"tpt large V {case}: loss err {el:.2e}, entropy err {eh:.2e}, dtext err {ed:.2e} of the largest entry")
    assert el <= LOSS_TOL and eh <= ENT_TOL and ed <= DT_TOL


# ------------------------------------------------------------------------------------------------------------ 3. ties
def test_ties_go_to_the_lower_view_index(dev):
    from clipfs import ops
    V, C, d, K = 16, 6, 64, 3
    F, T, _, _, H, sel = _ref(V, C, d, K, 0)
    order = torch.sort(H, stable=True).indices
    b = int(order[K - 1])  # the reference's last selected view
    rest = [int(u) for u in order[K:]]
    hi = [u for u in rest if u > b]
    lo = [u for u in rest if u < b]
    assert hi and lo, "the case must have unselected views on both sides of b"
    text = T.to(dev)
    # a copy of b's row above b: b stays, the copy stays out
    j = hi[0]
    Fa = F.clone()
    Fa[j] = F[b]
    _, s_a, _, e_a = ops.tpt_objective(Fa.to(dev)[None], text, K, S100, want_entropy=True)
    assert torch.equal(e_a[0, j], e_a[0, b])  # bitwise: a view's entropy does not depend on its index
    assert b in s_a[0].tolist() and j not in s_a[0].tolist() and sorted(s_a[0].tolist()) == sel.tolist()
    # a copy below b displaces it
    j = lo[0]
    Fb = F.clone()
    Fb[j] = F[b]
    _, s_b, _, e_b = ops.tpt_objective(Fb.to(dev)[None], text, K, S100, want_entropy=True)
    assert torch.equal(e_b[0, j], e_b[0, b])
    assert j in s_b[0].tolist() and b not in s_b[0].tolist()
    assert sorted(s_b[0].tolist()) == sorted([u for u in sel.tolist() if u != b] + [j])


# ---------------------------------------------------------------------------------------- 4. text and selection modes
def test_modes_are_bitwise_consistent(dev):
    from clipfs import ops
    V, C, d, K = 33, 130, 192, 3
    refs = [_ref(V, C, d, K, s) for s in (1, 2, 3)]
    feats = torch.stack([r[0] for r in refs]).to(dev)
    T = refs[0][1].to(dev)  # ONE text for the three images (images 2 and 3 are then foreign to it: still a valid input)
    loss, sel, dtext, ent = ops.tpt_objective(feats, T, K, S100, want_entropy=True)
    assert torch.isfinite(dtext).all() and torch.isfinite(loss).all()
    # run to run
    again = ops.tpt_objective(feats, T, K, S100, want_entropy=True)
    for a, b in zip((loss, sel, dtext, ent), again):
        assert torch.equal(a, b)
    # a text per image, three copies of the one
    l2, s2, d2, e2 = ops.tpt_objective(feats, T[None].repeat(3, 1, 1).contiguous(), K, S100, want_entropy=True)
    assert torch.equal(l2, loss) and torch.equal(s2, sel) and torch.equal(d2, dtext) and torch.equal(e2, ent)
    # the selection given back
    l3, s3, d3, e3 = ops.tpt_objective(feats, T, K, S100, selected=sel.clone())
    assert torch.equal(l3, loss) and torch.equal(s3, sel) and torch.equal(d3, dtext) and e3 is None
    # a given selection IS the selection: the three views of highest entropy, against the reference
    worst = torch.sort(torch.sort(refs[0][4]).indices[-K:]).values
    l4, _, d4, _ = ops.tpt_objective(feats[:1], T, K, S100, selected=worst.to(dev, torch.int32)[None].contiguous())
    rl, rd, _, _ = tpt_ref(refs[0][0], refs[0][1], K, S100, selected=worst)
    assert abs(l4.item() - rl.item()) <= LOSS_TOL
    assert (d4[0].double().cpu() - rd).abs().max().item() <= DT_TOL * rd.abs().max().item()
    # loss only
    l5, s5, d5, _ = ops.tpt_objective(feats, T, K, S100, want_grad=False)
    assert d5 is None and torch.equal(l5, loss) and torch.equal(s5, sel)
    # the gradient scale is exact for a power of two and reaches nothing else
    l6, _, d6, _ = ops.tpt_objective(feats, T, K, S100, grad_scale=4096.0)
    assert torch.equal(l6, loss) and torch.equal(d6, dtext * 4096.0)
    # an image's results do not depend on the batch around it
    for i in range(3):
        li, si, di, ei = ops.tpt_objective(feats[i:i + 1].contiguous(), T, K, S100, want_entropy=True)
        assert torch.equal(li[0], loss[i]) and torch.equal(si[0], sel[i]) and torch.equal(di[0], dtext[i])
        assert torch.equal(ei[0], ent[i])


def test_one_class_gives_zeros(dev):
    from clipfs import ops
    F, T = tpt_inputs(9, 1, 64, 0)
    loss, sel, dtext, ent = ops.tpt_objective(F.to(dev)[None].repeat(2, 1, 1), T.to(dev), 3, S100, want_entropy=True)
    assert (loss == 0).all() and (dtext == 0).all() and (ent == 0).all()
    assert sel.tolist() == [[0, 1, 2], [0, 1, 2]]  # every entropy ties: the lowest indices


# ------------------------------------------------------------------------------------------------- episodes: the model
NAMES = {"q": "q_proj", "k": "k_proj", "v": "v_proj"}


def _build(dev, cfg=None, r=4, sd_seed=11, C=5, max_len=12, backbone="small"):
    """A model with LoRA adapters (q, k, v of every block of both towers, weights from synth_lora) applied and FROZEN, a
    prompt learner over C synthetic captions, and the fp64 pieces of the oracle."""
    import lora_train_vlp as L
    import slow_pace as S
    from clipfs import synth
    from jclip.model import build_model
    from oracle import clip_oracle as O
    cfg = cfg or synth.SMALL
    sd = synth.synth_state_dict(cfg, seed=sd_seed, perturb=True)
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
    with torch.no_grad():
        for i, layer in enumerate(layers):
            for pr in "qkv":
                mod = getattr(layer, NAMES[pr])
                mod.w_lora_A.copy_(torch.from_numpy(lw[f"layer_{i}"][NAMES[pr]]["w_lora_A"]))
                mod.w_lora_B.copy_(torch.from_numpy(lw[f"layer_{i}"][NAMES[pr]]["w_lora_B"]))
    for n, prm in model.named_parameters():
        if "lora_" in n:
            prm.requires_grad_(False)
    model.eval()
    ids = synth.synth_captions(C, cfg.context_length, cfg.vocab_size, seed=4, max_len=max_len)
    learner = _learner(S, model, ids, dev)
    conv = lambda d: {p: {k: torch.from_numpy(v).double() for k, v in ab.items()} for p, ab in d.items()}
    tl = {b: conv(lw[f"layer_{b}"]) for b in range(cfg.transformer_layers)}
    return types.SimpleNamespace(L=L, O=O, cfg=cfg, model=model, learner=learner, ids=ids, layers=layers,
                                 sd64={k: v.double() for k, v in sd.items()}, tl=tl, sc=O.lora_scaling(1, r),
                                 ctx0=learner.ctx.detach().clone())


def _learner(S, model, ids, dev):
    learner = S.VLPromptLearner.__new__(S.VLPromptLearner)
    torch.nn.Module.__init__(learner)
    learner.ctx = torch.nn.Parameter(model.token_embedding.weight.data[ids[0, 1:5].to(dev)].clone())
    learner.tokenized_prompts, learner.n_ctx, learner.n_cls = ids.to(dev), 4, ids.shape[0]
    learner._model = [model]
    return learner


def _oracle_text(m, ctx64):
    """Unit class features [C, E] of the oracle's text tower for the prompt ctx ``ctx64`` (fp64, differentiable)."""
    O = m.O
    emb = O.build_prompts(ctx64, m.sd64["token_embedding.weight"], m.ids)
    return O.l2_normalize(O.encode_text(m.sd64, m.ids, m.tl, m.sc, embeds=emb))


def _episode_feats(T0, G, V, seed):
    """[G, V, E] fp32 unit view features around the mean class feature, with noise growing over a shuffled ramp: view
    entropies then differ by far more than the kernel's error, and the gradient is not ill-conditioned."""
    g = torch.Generator().manual_seed(seed)
    mean = T0.mean(0) / T0.mean(0).norm()
    out = []
    for _ in range(G):
        b = torch.linspace(0.05, 0.5, V, dtype=torch.float64)[torch.randperm(V, generator=g)]
        N = torch.randn(V, T0.shape[1], generator=g, dtype=torch.float64)
        F = mean[None] + b[:, None] * N / N.norm(dim=-1, keepdim=True)
        out.append(F / F.norm(dim=-1, keepdim=True))
    return torch.stack(out).float()


def _oracle_episode(m, F, K, s, selected=None):
    """(loss, ctx gradient, entropies, selection) of one image's first step in fp64."""
    ctx64 = m.ctx0.double().cpu().requires_grad_()
    T = _oracle_text(m, ctx64)
    loss, dT, H, sel = tpt_ref(F, T.detach(), K, s, selected=selected)
    T.backward(dT)
    return loss, ctx64.grad, H, sel


_SHARED = {}


def _small(dev):
    """The SMALL model of sections 5 and 6, its view features (G = 3, V = 8) and the first-step oracle per image; built
    once, read-only (the tests that change a flag put it back)."""
    if "small" not in _SHARED:
        m = _build(dev)
        with torch.no_grad():
            T0 = _oracle_text(m, m.ctx0.double().cpu())
        m.feats = _episode_feats(T0, 3, 8, seed=2)
        m.K = 2
        m.oracle = [_oracle_episode(m, m.feats[g], m.K, S100) for g in range(3)]
        m.dev_feats = m.feats.to(dev)
        _SHARED["small"] = m
    return _SHARED["small"]


def _tuner(m, **kw):
    from tpt import TestTimePromptTuner
    kw.setdefault("rho", 0.25)  # 8 views: K = 2
    return TestTimePromptTuner(m.model, m.learner, **kw)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ----------------------------------------------------------------------------- 5. an episode against the fp64 oracle
def test_episode_matches_oracle(dev):
    m = _small(dev)
    res = _tuner(m).adapt_features(m.dev_feats)
    G, C = 3, m.ids.shape[0]
    assert tuple(res.logits.shape) == (G, C) and tuple(res.ctx.shape) == (G,) + tuple(m.ctx0.shape)
    assert tuple(res.loss.shape) == (G, 1) and tuple(res.selected.shape) == (G, m.K) and tuple(res.entropy.shape) == (G, 8)
    worst_g = worst_l = 0.0
    for g in range(G):
        loss, grad, H, sel = m.oracle[g]
        assert entropy_gap(H, m.K) >= 5e-3  # on the oracle: the selection is well separated
        assert res.selected[g].tolist() == sel.tolist()
        got = res.ctx_grad[g].double().cpu()
        worst_g = max(worst_g, (got - grad).abs().max().item() / grad.abs().max().item())
        # AdamW from zero moments, step 1, on the ENGINE's gradient (the first step is nearly lr * sign(g))
        want, _, _ = m.O.jt_adamw_step(m.ctx0.double().cpu(), got, torch.zeros_like(got), torch.zeros_like(got), 1,
                                       lr=5e-3, weight_decay=0.01)
        assert (res.ctx[g].double().cpu() - want).abs().max().item() < 1e-6
        # the final logits against the oracle AT THE ENGINE'S tuned ctx
        with torch.no_grad():
            Tt = _oracle_text(m, res.ctx[g].double().cpu())
        ref = S100 * m.feats[g, 0].double() @ Tt.t()
        worst_l = max(worst_l, (res.logits[g].double().cpu() - ref).abs().max().item())
        assert grad.abs().max().item() > 1e-4
    print(f"tpt episode: ctx_grad err {worst_g:.2e} of the largest entry, final logits err {worst_l:.2e}")
    assert worst_g <= CTX_GRAD_TOL and worst_l <= EP_LOGIT_TOL


# --------------------------------------------------------------- 6. episodes leave no trace and share one forward
def _slots(m):
    out = []
    for tower in (m.model.transformer, m.model.visual.transformer):
        for blk in tower.resblocks:
            out.extend(g for _, g in blk.attn.trainable_pairs())
    return out


def test_group_is_bitwise_the_single_episodes_and_leaves_no_trace(dev):
    m = _small(dev)
    tuner = _tuner(m)
    eng = m.model.engine
    for s in _slots(m):
        s.fill_(0.5)
    m.learner.ctx.grad = torch.full_like(m.learner.ctx.data, 0.25)
    keep = [m.learner.ctx.detach().clone(), m.learner.ctx.grad.clone(), eng.step] + [s.clone() for s in _slots(m)]
    try:
        whole = tuner.adapt_features(m.dev_feats)
        singles = [tuner.adapt_features(m.dev_feats[g:g + 1].contiguous()) for g in range(3)]
        for g in range(3):  # the shared first forward: a group is bitwise its episodes run alone
            assert _same([t[g:g + 1] for t in whole], singles[g])
        # an episode leaves nothing behind for the next one: b after a is b alone
        assert _same(tuner.adapt_features(m.dev_feats[1:2].contiguous()), singles[1])
        now = [m.learner.ctx.detach(), m.learner.ctx.grad, eng.step] + _slots(m)
        assert now[2] == keep[2] and m.model.engine is eng
        assert all(torch.equal(a, b) for a, b in zip(now[:2] + now[3:], keep[:2] + keep[3:]))
    finally:
        m.learner.ctx.grad = None
        for s in _slots(m):
            s.zero_()


def test_two_steps_reuse_the_selection(dev):
    m = _small(dev)
    one = _tuner(m).adapt_features(m.dev_feats)
    two = _tuner(m, steps=2).adapt_features(m.dev_feats)
    assert tuple(two.loss.shape) == (3, 2) and torch.isfinite(two.loss).all() and torch.isfinite(two.logits).all()
    assert torch.equal(two.selected, one.selected) and torch.equal(two.loss[:, 0], one.loss[:, 0])
    assert torch.equal(two.ctx_grad, one.ctx_grad) and torch.equal(two.entropy, one.entropy)
    assert not torch.equal(two.ctx, one.ctx) and not torch.equal(two.loss[:, 1], one.loss[:, 0])


def test_no_host_synchronisation(dev):
    m = _small(dev)
    tuner = _tuner(m, steps=2)
    tuner.adapt_features(m.dev_feats)  # warm-up: the text tower's row plan of this prompt table, the workspaces
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        res = tuner.adapt_features(m.dev_feats)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(res.logits).all()


# --------------------------------------------------------------------- 7. image towers, precision modes and refusals
def test_views_through_a_vit_tower(dev):
    """adapt_views = the no-grad image pass + adapt_features, and it does not advance the dropout seed counter."""
    from clipfs import ops, synth
    m = _small(dev)
    views = synth.synth_images(2 * 5, m.cfg.image_resolution, seed=3).reshape(2, 5, 3, m.cfg.image_resolution,
                                                                              m.cfg.image_resolution).to(dev)
    tuner = _tuner(m, rho=0.4)
    step = m.model.engine.step
    res = tuner.adapt_views(views)
    f, _ = m.model.engine.vit_forward(views.reshape(10, *views.shape[2:]), False, 0)
    assert _same(res, tuner.adapt_features(ops.l2norm_fwd(f).reshape(2, 5, -1)))
    assert m.model.engine.step == step and tuple(res.selected.shape) == (2, 2)


def test_modified_resnet_tower_end_to_end(dev):
    import modified_resnet_ref as R
    import slow_pace as S
    from clipfs import ops, synth
    from jclip.model import build_model
    from oracle import clip_oracle as O
    geo = R.geometries()["RN_TINY"]
    sd = R.synth_sd(geo)
    model = build_model(sd, device=dev)
    ids = synth.synth_captions(6, geo.text.context_length, geo.text.vocab_size, seed=4, max_len=10)
    learner = _learner(S, model, ids, dev)
    m = types.SimpleNamespace(O=O, ids=ids, sd64=R.to64(sd), tl=None, sc=0.0, ctx0=learner.ctx.detach().clone())
    G, V, K, s = 2, 8, 2, S100
    views = synth.synth_images(G * V, geo.resolution, seed=3).reshape(G, V, 3, geo.resolution, geo.resolution).to(dev)
    from tpt import TestTimePromptTuner
    tuner = TestTimePromptTuner(model, learner, rho=0.25)
    res = tuner.adapt_views(views)
    feats = ops.l2norm_fwd(model.engine.vit_forward(views.reshape(G * V, *views.shape[2:]), False, 0)[0]).reshape(G, V, -1)
    worst = 0.0
    for g in range(G):
        # The oracle given the engine's image features and its selection: a random ResNet maps these synthetic views to
        # features 1e-4 apart, so their entropies lie closer together (4e-4 at K) than the fp32 text tower's logits are to
        # the oracle's (1e-3, the bound of smoke()).  The set must still be one the oracle's entropies allow within that.
        loss, grad, H, _ = _oracle_episode(m, feats[g].cpu(), K, s, selected=res.selected[g])
        hk = torch.sort(H).values[K - 1].item()
        inside = torch.zeros(V, dtype=torch.bool)
        inside[res.selected[g].long().cpu()] = True
        assert (H[inside] <= hk + ENT_TOL + 1e-3).all() and (H[~inside] >= hk - ENT_TOL - 1e-3).all()
        assert grad.abs().max().item() > 1e-4
        worst = max(worst, (res.ctx_grad[g].double().cpu() - grad).abs().max().item() / grad.abs().max().item())
    print(f"tpt ModifiedResNet episode: ctx_grad err {worst:.2e} of the largest entry")
    assert torch.isfinite(res.logits).all() and worst <= RN_CTX_GRAD_TOL


def test_fp16_storage_mode_episode_with_a_loss_scale(dev):
    """The geometry of test_fp16_storage_mode_step_with_a_scale (ViT-L/14 widths, depth 2 + 2, rank 16): the fp16 storage
    mode's ctx gradient under loss_scale 4096 against the fp32 episode's."""
    from clipfs import synth
    cfg = dataclasses.replace(synth.VIT_L14, vision_layers=2, transformer_layers=2, vocab_size=2048)
    m = _build(dev, cfg=cfg, backbone="ViT-L/14", r=16, sd_seed=17, C=6, max_len=20)
    with torch.no_grad():
        T0 = _oracle_text(m, m.ctx0.double().cpu())
    feats = _episode_feats(T0, 2, 8, seed=2)
    for g in range(2):  # on the oracle: the gap at K is several times the 1e-2 the fp16 storage mode may move a logit by
        assert entropy_gap(_oracle_episode(m, feats[g], 2, S100)[2], 2) >= 4e-2
    feats = feats.to(dev)
    a = _tuner(m).adapt_features(feats)
    scaled = _tuner(m, loss_scale=4096.0).adapt_features(feats)
    assert torch.equal(scaled.ctx_grad, a.ctx_grad) and torch.equal(scaled.ctx, a.ctx)  # fp32: a power of two is exact
    m.model.engine.precision = "fp16"
    b = _tuner(m, loss_scale=4096.0).adapt_features(feats)
    rmax = a.ctx_grad.abs().max().item()
    err = (b.ctx_grad - a.ctx_grad).abs().max().item()
    print(f"tpt fp16 storage mode, loss_scale 4096: ctx_grad err {err:.3e} of the largest fp32 entry {rmax:.3e} "
          f"(ratio {err / rmax:.2e})")
    assert torch.isfinite(b.ctx_grad).all() and torch.isfinite(b.logits).all() and rmax > 1e-5
    assert torch.equal(b.selected, a.selected)
    assert err <= FP16_CTX_GRAD_TOL * rmax


def test_refusals_on_the_device(dev):
    from clipfs import ops
    m = _small(dev)
    tuner = _tuner(m)
    with pytest.raises(ValueError, match="1025 views"):
        tuner.adapt_features(torch.zeros(1, 1025, m.cfg.embed_dim, device=dev))
    with pytest.raises(_lib_error(), match="views 1025"):
        ops.tpt_objective(torch.zeros(1, 1025, 64, device=dev), torch.zeros(3, 64, device=dev), 6)
    a = m.model.transformer.resblocks[0].attn
    params = [p for p, _ in a.trainable_pairs()]
    try:
        for p in params:
            p.requires_grad_(True)
        with pytest.raises(ValueError, match=r"requires_grad_\(False\)"):
            tuner.adapt_features(m.dev_feats)
    finally:
        for p in params:
            p.requires_grad_(False)
    try:
        assert m.L.merge_lora(m.model) > 0
        with pytest.raises(ValueError, match="merged"):
            tuner.adapt_features(m.dev_feats)
        with pytest.raises(ValueError, match="merged"):
            _tuner(m)
    finally:
        m.L.unmerge_lora(m.model)
    assert _same(tuner.adapt_features(m.dev_feats[:1].contiguous()), tuner.adapt_features(m.dev_feats[:1].contiguous()))


def _lib_error():
    from clipfs._lib import ClipfsError
    return ClipfsError
