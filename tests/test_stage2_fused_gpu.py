"""The fused stage-2 step on the GPU (``Stage2Trainer(..., fused=True)``): the objective kernel against the fp64 oracle
pieces, the fused step against the oracle and against the unfused trainer (eval mode and dropout 0.25: the seed
order), deep prompts, two data-parallel ranks on the one GPU against the single-process step, and loss scaling held to
what tests/test_loss_scale_gpu.py holds LoRATrainer to.  Models: synth.SMALL with rank-4 LoRA applied and frozen,
4 ctx + 4 VPT tokens, built as tests/test_stage2.py::test_stage2_trainer_step_matches_oracle builds its own."""
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

NAMES = {"q": "q_proj", "k": "k_proj", "v": "v_proj"}
ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _paths():
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for path in (os.path.join(root, "jittor-clip-fewshot_amd"), root):
        if path not in sys.path:
            sys.path.insert(0, path)


def _unit(t):
    return t / t.norm(dim=-1, keepdim=True)


# ---------------------------------------------------------------------------------------------------- 1. the kernel
# the issue's shapes (B, C, d, C_loc), then three of this file's: C a multiple of 4 (the float4 logits rows, one and
# several passes of the wave) and an empty class block
SHAPES = [(3, 5, 7, 5), (16, 11, 64, 4), (2, 403, 512, 403), (65, 130, 33, 1), (1, 1, 4, 1),
          (9, 64, 16, 7), (6, 260, 36, 260), (5, 12, 8, 0)]


def _kernel_inputs(B, C, d, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    img = _unit(r(B, d)).float()
    txt = _unit(r(C, d)).float()
    zs_img = _unit(img.double() + 0.3 * r(B, d)).float()
    zs_txt = _unit(txt.double() + 0.3 * r(C, d)).float()
    zs_img[0, :min(3, d)] = img[0, :min(3, d)]   # exact ties: sign(0) = 0
    zs_txt[0, :min(2, d)] = txt[0, :min(2, d)]
    cos = (100.0 * img.double() @ txt.double().t()).float()
    zs_logits = (100.0 * zs_img.double() @ zs_txt.double().t()).float()
    target = torch.randint(0, C, (B,), generator=g)
    return img, txt, zs_img, zs_txt, cos, zs_logits, target


def _oracle_pieces(x, C_loc):
    from oracle import clip_oracle as O
    img, txt, zs_img, zs_txt, cos, zs_logits, target = x
    C = txt.shape[0]
    cos64, img64 = cos.double().requires_grad_(), img.double().requires_grad_()
    txt64 = txt[:C_loc].double().requires_grad_()
    terms = [O.jt_cross_entropy(cos64, target), O.scl_logits_loss(cos64, zs_logits.double()),
             O.jt_l1_loss(img64, zs_img.double())]
    # the C_loc rows' share of mean |txt - zs_txt| over all C rows
    terms.append(O.jt_l1_loss(txt64, zs_txt[:C_loc].double()) * C_loc / C if C_loc else torch.zeros((), dtype=torch.float64))
    sum(terms).backward()
    return [t.item() for t in terms], cos64.grad, img64.grad, (txt64.grad if C_loc else None)


# offset 1 puts every float operand one float past a 16-byte boundary, so a shape with a float4 path (C or d a multiple
# of 4) takes its scalar rows there; the other shapes run the scalar rows anyway
CASES = [(s, 0) for s in SHAPES] + [(s, 1) for s in SHAPES if s[1] % 4 == 0 or s[2] % 4 == 0]


@pytest.mark.parametrize("shape,offset", CASES)
def test_objective_kernel_matches_oracle_pieces(dev, shape, offset):
    from clipfs import ops
    B, C, d, C_loc = shape
    x = _kernel_inputs(B, C, d, seed=B * 1000 + C)
    want_terms, want_dcos, want_dimg, want_dtxt = _oracle_pieces(x, C_loc)

    def put(t):  # a contiguous device copy whose base is `offset` floats past a 256-byte aligned allocation
        buf = torch.empty(t.numel() + offset, device=dev)
        v = buf[offset:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 * offset
        return v

    img, txt, zs_img, zs_txt, cos, zs_logits, target = x
    a = dict(cos=put(cos), zs_logits=put(zs_logits), target=target.to(dev), img=put(img), zs_img=put(zs_img),
             txt=put(txt[:C_loc]) if C_loc else None, zs_txt=put(zs_txt[:C_loc]) if C_loc else None, classes=C,
             inv_global_batch=1.0 / B)
    terms, correct, dcos, dimg, dtxt = ops.stage2_objective(**a)
    got = terms.cpu().double().tolist()
    for name, g, w in zip(("sim_ce", "scl_logits", "scl_image", "scl_text"), got, want_terms):
        print(f"{shape} +{offset}: {name} {g:.8e} oracle {w:.8e} rel {abs(g - w) / max(1.0, abs(w)):.2e}")
        assert abs(g - w) < 2e-5 * max(1.0, abs(w)), name
    assert correct.item() == int((cos.argmax(1) == target).sum())
    for name, g, w in (("dcos", dcos, want_dcos), ("dimg", dimg, want_dimg), ("dtxt", dtxt, want_dtxt)):
        if w is None:
            assert g is None
            continue
        err, big = (g.cpu().double() - w).abs().max().item(), w.abs().max().item()
        print(f"{shape} +{offset}: {name} max err {err:.2e} of largest entry {big:.2e}")
        assert err <= 2e-4 * max(big, 1e-12), name
    if C_loc:  # exact ties carry no gradient
        assert (dtxt[0, :min(2, d)] == 0).all()
    assert (dimg[0, :min(3, d)] == 0).all()
    # a static scale of 1024 (read from the device record): gradients bitwise 1024 x, terms and count unchanged
    st = ops.new_scaler_state(1024.0, dev)
    terms_s, correct_s, dcos_s, dimg_s, dtxt_s = ops.stage2_objective(**a, scale_state=st)
    assert torch.equal(terms_s, terms) and torch.equal(correct_s, correct)
    assert torch.equal(dcos_s, dcos * 1024.0) and torch.equal(dimg_s, dimg * 1024.0)
    assert dtxt is None or torch.equal(dtxt_s, dtxt * 1024.0)
    # run to run
    again = ops.stage2_objective(**a)
    for p, q in zip((terms, correct, dcos, dimg, dtxt), again):
        assert (p is None and q is None) or torch.equal(p, q)
    # without gradients: the same terms
    t2, c2, n1, n2, n3 = ops.stage2_objective(**a, want_grad=False)
    assert n1 is None and n2 is None and n3 is None and torch.equal(t2, terms) and torch.equal(c2, correct)


def test_objective_kernel_global_batch_and_label_outside_range(dev):
    """inv_global_batch is the only place the batch size enters (a shard of a larger batch); a label outside [0, C) reads
    nothing and turns its row's loss into NaN."""
    from clipfs import ops
    B, C, d = 4, 6, 8
    img, txt, zs_img, zs_txt, cos, zs_logits, target = (t.to(dev) for t in _kernel_inputs(B, C, d, seed=5))
    one = ops.stage2_objective(cos, zs_logits, target, img, zs_img, txt, zs_txt, C, 1.0 / B)
    four = ops.stage2_objective(cos, zs_logits, target, img, zs_img, txt, zs_txt, C, 1.0 / (4 * B))
    assert torch.equal(four[0][:3], one[0][:3] * 0.25) and torch.equal(four[0][3], one[0][3])
    assert torch.equal(four[2], one[2] * 0.25) and torch.equal(four[3], one[3] * 0.25) and torch.equal(four[4], one[4])
    bad = target.clone()
    bad[1] = C
    terms, correct, dcos, _, _ = ops.stage2_objective(cos, zs_logits, bad, img, zs_img, txt, zs_txt, C, 1.0 / B)
    assert torch.isnan(terms[0]) and torch.isfinite(terms[1:]).all() and torch.isfinite(dcos).all()


# ------------------------------------------------------------------------------------------------- model and trainer
def _design(depth):
    if depth <= 1:
        return {"vision_ctx": 4}
    return {"vision_ctx": 4, "language_ctx": 4, "deep_prompts": True, "vision_depth": depth, "language_depth": depth}


def _setup(dev, p=0.0, depth=1, B=6, C=5, cfg=None, backbone="small", r=4, sd_seed=11, max_len=12, **kw):
    """Model + learner + head + data as the oracle test of tests/test_stage2.py builds them; LoRA applied and frozen.
    ``kw`` goes to Stage2Trainer; returns a namespace with the trainer ``tr``."""
    _paths()
    import lora_train_vlp as L
    import slow_pace as S
    from clipfs import synth
    from jclip.model import build_model
    cfg = cfg or synth.SMALL
    sd = synth.synth_state_dict(cfg, seed=sd_seed, perturb=True)
    model = build_model(sd, design_details=_design(depth), device=dev)
    args = types.SimpleNamespace(encoder="both", position="all", backbone=backbone, params=["q", "k", "v"], r=r, alpha=1,
                                 dropout_rate=p)
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
    for n, prm in model.named_parameters():  # stage 2: LoRA applied but frozen (slow_pace.py:1551-1556)
        if "lora_" in n:
            prm.requires_grad_(False)
    model.train(p > 0)
    d = cfg.embed_dim
    g = torch.Generator().manual_seed(1)
    images = synth.synth_images(B, cfg.image_resolution, seed=3)
    target = synth.synth_labels(B, C, seed=2)
    zs_img = _unit(torch.randn(B, d, generator=g, dtype=torch.float64))
    zs_txt = _unit(torch.randn(C, d, generator=g, dtype=torch.float64))
    ids = synth.synth_captions(C, cfg.context_length, cfg.vocab_size, seed=4, max_len=max_len)
    learner = S.VLPromptLearner.__new__(S.VLPromptLearner)
    torch.nn.Module.__init__(learner)
    learner.ctx = torch.nn.Parameter(model.token_embedding.weight.data[ids[0, 1:5].to(dev)].clone())
    learner.tokenized_prompts, learner.n_ctx, learner.n_cls = ids.to(dev), 4, C
    learner._model = [model]
    head = S.Channel_LP(d, C, device=dev)
    with torch.no_grad():
        head.fc.weight.copy_(zs_txt.float())
        head.scale1.copy_(1 + 0.1 * torch.randn(d, generator=g))
        head.fc.bias.copy_(0.01 * torch.randn(C, generator=g))  # nn.Linear's own draw comes from the global generator
    tr = S.Stage2Trainer(model, learner, head, zs_img, zs_txt, lr=1e-3, total_epoch=20, **kw)
    return types.SimpleNamespace(S=S, cfg=cfg, sd=sd, lw=lw, model=model, learner=learner, head=head, tr=tr, ids=ids,
                                 images=images.to(dev), target=target.to(dev), index=torch.arange(B), zs_img=zs_img,
                                 zs_txt=zs_txt, B=B, C=C)


def _named(s):
    """{name: parameter} of everything the trainers train, under names both trainers share."""
    out = {"ctx": s.learner.ctx, "VPT": s.model.visual.VPT}
    out.update({n: p for n, p in s.model.named_parameters() if n.endswith(".VPT_shallow")})
    out.update({"head." + n: p for n, p in s.head.named_parameters()})
    return out


def _grad(s, p):
    return (p.grad_slot if s.tr.fused else p.grad).detach().clone()


def _step(s):
    return s.tr.step(s.images, s.target, s.index)


# --------------------------------------------------------------------------------------- 2. fused step against the oracle
def test_fused_step_matches_oracle(dev):
    from oracle import clip_oracle as O
    import test_engine_gpu as T
    s = _setup(dev, fused=True)
    tr = s.tr
    assert isinstance(tr, s.S.FusedStage2Trainer) and tr.fused and (tr.rank, tr.world, tr.collectives_per_step) == (0, 1, 0)
    assert tr.flat.numel == sum(p.numel() for p in tr.params) and tr.loss_scale_value is None
    p0 = [p.detach().clone() for p in tr.params]
    loss, terms, cos = _step(s)
    assert tr.last_plan == {"text": 0, "vision": 0} and (tr.t, tr.optimizer_steps, tr.skipped_steps) == (1, 1, 0)
    C, cfg = s.C, s.cfg
    sd64 = {k: v.double() for k, v in s.sd.items()}
    tl, vl = T._oracle_lora(s.lw, cfg)
    sc = O.lora_scaling(1, 4)
    ctx64 = p0[0].double().cpu().requires_grad_()
    vpt64 = p0[1].double().cpu().requires_grad_()
    emb = sd64["token_embedding.weight"][s.ids]
    prompts = torch.cat([emb[:, :1], ctx64.unsqueeze(0).expand(C, -1, -1), emb[:, 5:]], dim=1)   # slow_pace.py:185-199
    txt = O.encode_text(sd64, s.ids, tl, sc, embeds=prompts)
    img = O.encode_image(sd64, s.images.double().cpu(), vl, sc, vpt=vpt64)
    lp64 = [t.double().cpu().requires_grad_() for t in p0[2:]]
    ref, rterms, rcos = O.stage2_loss(img, txt, s.target.cpu(), s.zs_img, s.zs_txt, tuple(lp64), img.detach(), s.zs_txt)
    ref.backward()
    print(f"loss {loss.item():.8f} oracle {ref.item():.8f} rel {abs(loss.item() - ref.item()) / abs(ref.item()):.2e}")
    assert abs(loss.item() - ref.item()) < 5e-5 * abs(ref.item())
    for k, v in rterms.items():
        assert abs(terms[k].item() - v.item()) < 5e-5 * max(1.0, abs(v.item())), k
    assert (cos.cpu().double() - rcos.detach()).abs().max() < 1e-3
    want = [ctx64.grad, vpt64.grad] + [t.grad for t in lp64]
    for p, w in zip(tr.params, want):
        err = (p.grad_slot.detach().cpu().double() - w).abs().max().item()
        print(f"grad {tuple(w.shape)}: max err {err:.2e} of largest entry {w.abs().max().item():.2e}")
        assert err <= 5e-4 * max(w.abs().max().item(), 1e-6)
    # AdamW with the pre-step learning rate, then the cosine schedule advanced once (:1696-1697)
    assert abs(tr.lr - O.cosine_annealing_lr(1e-3, 1, 20)) < 1e-12
    for p, q, w in zip(tr.params, p0, want):
        q64 = q.double().cpu()
        exp, _, _ = O.jt_adamw_step(q64, w, torch.zeros_like(q64), torch.zeros_like(q64), 1, lr=1e-3, weight_decay=1e-2)
        assert (p.detach().cpu().double() - exp).abs().max().item() < 1e-6
    # the head still works as a module on its re-homed parameters
    out = s.head(torch.randn(3, cfg.embed_dim, device=dev))
    lo = tr.flat.params.data_ptr()
    assert out.shape == (3, C) and all(lo <= q.data_ptr() < lo + 4 * tr.flat.numel for q in s.head.parameters())


# ------------------------------------------------------------------------------------------ 3. fused against unfused
@pytest.mark.parametrize("p", [0.0, 0.25])
def test_fused_matches_unfused(dev, p):
    """Same parameters, same engine seed state.  Train mode at dropout 0.25 is what checks the seed order (text, image,
    second image): a swapped pair would put other masks on the same batch.  After three steps the
    parameters are held to 3 x (1e-6 + 1e-6): each trainer's AdamW step is within 1e-6 of the oracle's."""
    a, b = _setup(dev, p=p, fused=True), _setup(dev, p=p)
    assert a.model.training == (p > 0) and not b.tr.fused
    na, nb = _named(a), _named(b)
    for k in na:
        assert torch.equal(na[k].detach(), nb[k].detach()), k
    for step in range(3):
        la, ta, ca = _step(a)
        lb, tb, cb = _step(b)
        if step == 0:
            print(f"p={p}: loss fused {la.item():.8f} unfused {lb.item():.8f}")
            assert abs(la.item() - lb.item()) < 5e-5 * abs(lb.item())
            assert (ca - cb).abs().max().item() < 1e-3
            for k in tb:
                assert abs(ta[k].item() - tb[k].item()) < 5e-5 * max(1.0, abs(tb[k].item())), k
            for k in na:
                ga, gb = _grad(a, na[k]), _grad(b, nb[k])
                err, big = (ga - gb).abs().max().item(), gb.abs().max().item()
                print(f"p={p}: grad {k}: max diff {err:.2e} of largest entry {big:.2e}")
                assert err <= 5e-4 * max(big, 1e-6), k
    assert abs(a.tr.lr - b.tr.lr) < 1e-15 and a.tr.t == b.tr.t == 3
    assert a.model.engine.step == b.model.engine.step == (9 if p > 0 else 0)
    for k in na:
        err = (na[k].detach() - nb[k].detach()).abs().max().item()
        print(f"p={p}: after 3 steps {k}: max diff {err:.2e}")
        assert err < 3 * 2e-6, k


# --------------------------------------------------------------------------------------------------- 4. deep prompts
def test_fused_deep_prompts_match_unfused(dev):
    a, b = _setup(dev, depth=2, fused=True), _setup(dev, depth=2)
    na, nb = _named(a), _named(b)
    deep = [k for k in na if k.endswith(".VPT_shallow")]
    assert len(deep) == 2 and len(a.tr.flat.deep_prompts) == 2  # block 1 of each tower
    before = {k: na[k].detach().clone() for k in deep}
    la, _, _ = _step(a)
    lb, _, _ = _step(b)
    assert abs(la.item() - lb.item()) < 5e-5 * abs(lb.item())
    flat = a.tr.flat
    lo, hi = flat.grads.data_ptr(), flat.grads.data_ptr() + 4 * flat.numel
    for k in na:
        ga, gb = _grad(a, na[k]), _grad(b, nb[k])
        err, big = (ga - gb).abs().max().item(), gb.abs().max().item()
        print(f"deep: grad {k}: max diff {err:.2e} of largest entry {big:.2e}")
        assert err <= 5e-4 * max(big, 1e-6), k
        assert lo <= na[k].grad_slot.data_ptr() < hi and big > 0  # a slot of the flat buffer, and it received something
    for k in deep:
        assert not torch.equal(na[k].detach(), before[k])
        assert (na[k].detach() - nb[k].detach()).abs().max().item() < 2e-6


# ------------------------------------------------------------------------------------------------------ 5. two ranks
BG, CG = 7, 5  # shards of 4 + 3 images and 3 + 2 classes


def _free_port():
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    return port


def _dp_rank_main(rank, world, port, shard_text, out_dir, p):
    _paths()
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    from clipfs import dist as D
    dev = torch.device("cuda:0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    s = _setup(dev, p=p, B=BG, C=CG, fused=True, process_group=dist.group.WORLD, shard_text=shard_text)
    tr = s.tr
    assert (tr.rank, tr.world) == (rank, world) and tr.collectives_per_step == (4 if shard_text else 2)
    lo, hi = D.block_bounds(BG, rank, world)
    assert hi - lo == (4, 3)[rank] and D.block_bounds(CG, rank, world) == ((0, 3), (3, 5))[rank]
    tr.time_collectives = True
    loss, terms, cos = tr.step(s.images[lo:hi].contiguous(), s.target[lo:hi].contiguous(), s.index[lo:hi], 0, BG, lo)
    torch.cuda.synchronize()
    names = sorted(tr.collective_times_ms())
    assert names == (["all_gather", "all_gather_head", "all_reduce", "reduce_scatter"] if shard_text
                     else ["all_gather_head", "all_reduce"]), names
    assert cos.shape == (hi - lo, CG)
    if rank != 0:  # terms that exist once per step are rank 0's
        assert terms["lp_ce"].item() == 0.0 and (shard_text or terms["scl_text"].item() == 0.0)
    total = torch.stack([loss] + [terms[k] for k in sorted(terms)]).clone()
    D.allreduce_sum_(total)
    torch.cuda.synchronize()
    np.savez(os.path.join(out_dir, f"dp{rank}.npz"), grads=tr.flat.grads.cpu().numpy(), params=tr.flat.params.cpu().numpy(),
             total=total.cpu().numpy())
    dist.destroy_process_group()


@pytest.mark.parametrize("shard_text,p", [(True, 0.0), (False, 0.0), (True, 0.25)])
def test_two_ranks_match_single_process(dev, tmp_path, shard_text, p):
    s = _setup(dev, p=p, B=BG, C=CG, fused=True)
    loss, terms, _ = _step(s)
    want_g, want_p = s.tr.flat.grads.cpu().numpy(), s.tr.flat.params.cpu().numpy()
    want_total = np.array([loss.item()] + [terms[k].item() for k in sorted(terms)])
    ctx = mp.spawn(_dp_rank_main, args=(2, _free_port(), shard_text, str(tmp_path), p), nprocs=2, join=False)
    deadline = time.monotonic() + 120  # a rank that hangs is killed, not waited for
    try:
        while not ctx.join(timeout=5):
            assert time.monotonic() < deadline, "a data-parallel rank did not finish in time"
    finally:
        for proc in ctx.processes:
            if proc.is_alive():
                proc.kill()
    z = [np.load(os.path.join(str(tmp_path), f"dp{r}.npz")) for r in range(2)]
    scale = np.abs(want_g).max()
    assert scale > 1e-5
    for r in range(2):  # test_dp_gpu._compare's budgets
        eg, ep = np.abs(z[r]["grads"] - want_g).max(), np.abs(z[r]["params"] - want_p).max()
        print(f"shard_text={shard_text} p={p} rank {r}: grad diff {eg:.2e} of {scale:.2e}, param diff {ep:.2e}, "
              f"loss {z[r]['total'][0]:.7f} vs {want_total[0]:.7f}")
        assert eg < 2e-5 * scale + 1e-9
        assert ep < 1e-6
        assert np.abs(z[r]["total"] - want_total).max() < 1e-4  # the loss and each of its terms, summed over the ranks
    assert np.array_equal(z[0]["params"].view(np.int32), z[1]["params"].view(np.int32))


# --------------------------------------------------------------------------------------------------- 6. loss scaling
LR = 1e-3
ADAMW_TOL = 4 * LR * ULP  # tests/test_loss_scale_gpu.py: one ulp on each of the two device-computed bias corrections


@pytest.fixture(scope="module")
def unscaled(dev):
    """Three unscaled fused steps: the gradient of the first, the parameters after each (computed once, left alone)."""
    s = _setup(dev, fused=True)
    out = dict(params=[])
    for i in range(3):
        _step(s)
        if i == 0:
            out["grad"] = s.tr.flat.grads.clone()
        out["params"].append(s.tr.flat.params.clone())
    assert s.tr.optimizer_steps == s.tr.t == 3 and s.tr.skipped_steps == 0 and s.tr.loss_scale_value is None
    return out


@pytest.mark.parametrize("mode", ["static", "dynamic"])
def test_scaled_steps_equal_unscaled_steps(dev, unscaled, mode):
    """A power-of-two scale is exact in fp32; under "dynamic" the scale doubles after growth_interval = 2 clean steps."""
    kw = dict(loss_scale=2.0 ** 12) if mode == "static" else dict(loss_scale="dynamic", init_scale=2.0 ** 12,
                                                                  growth_interval=2)
    s = _setup(dev, fused=True, **kw)
    tr = s.tr
    want_g = unscaled["grad"]
    gmax = want_g.abs().max().item()
    assert gmax > 1e-5
    scales = [tr.loss_scale_value]
    for i in range(3):
        _step(s)
        if i == 0:
            err = (tr.flat.grads * 2.0 ** -12 - want_g).abs().max().item()
            print(f"{mode}: max |grad * 2^-12 - unscaled grad| = {err:.3e} of largest entry {gmax:.3e}")
            assert err <= 1e-4 * gmax
        scales.append(tr.loss_scale_value)
        err = (tr.flat.params - unscaled["params"][i]).abs().max().item()
        print(f"{mode}: step {i + 1}: max |param - unscaled| = {err:.3e} (bound {(i + 1) * ADAMW_TOL:.3e})")
        assert err <= (i + 1) * ADAMW_TOL
    assert (tr.optimizer_steps, tr.skipped_steps, tr.t) == (3, 0, 3)
    assert scales == ([4096.0] * 4 if mode == "static" else [4096.0, 4096.0, 8192.0, 8192.0])


@pytest.mark.parametrize("mode", ["static", "dynamic"])
def test_skip_path(dev, mode):
    """Gradients made non-finite by an input (an inf written into the buffer before the optimiser step, as
    tests/test_loss_scale_gpu.py does): nothing moves, the step is counted as skipped, the cosine schedule advances."""
    from oracle import clip_oracle as O
    kw = dict(loss_scale=65536.0) if mode == "static" else dict(loss_scale="dynamic")
    s = _setup(dev, fused=True, **kw)
    tr = s.tr
    assert tr.loss_scale_value == 65536.0
    tr.flat.zero_grad()
    tr.forward_backward(s.images, s.target, s.index)
    assert torch.isfinite(tr.flat.grads).all()
    keep = [x.clone() for x in (tr.flat.params, tr.flat.m, tr.flat.v)]
    tr.flat.grads[tr.flat.numel // 2] = float("inf")
    tr.optimizer_step()
    for got, want in zip((tr.flat.params, tr.flat.m, tr.flat.v), keep):
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    after = 32768.0 if mode == "dynamic" else 65536.0
    assert (tr.skipped_steps, tr.optimizer_steps, tr.t, tr.loss_scale_value) == (1, 0, 1, after)
    assert abs(tr.lr - O.cosine_annealing_lr(LR, 1, 20)) < 1e-12  # the schedule counts iterations
    _step(s)  # the next clean step is AdamW's step 1
    assert (tr.skipped_steps, tr.optimizer_steps, tr.t, tr.loss_scale_value) == (1, 1, 2, after)
    assert not torch.equal(tr.flat.params, keep[0])


def test_fp16_storage_mode_step_with_a_scale(dev):
    """One fused step in the fp16 storage mode under loss_scale 2^12 against the fp32 fused step, at the ViT-L/14 shapes
    (depth 2 + 2, rank 16) and within the budget tests/test_loss_scale_gpu.py / test_fp16_precision_mode_l14 grant the
    two modes: 3e-2 of the largest gradient entry."""
    from clipfs import synth
    cfg = dataclasses.replace(synth.VIT_L14, vision_layers=2, transformer_layers=2, vocab_size=2048)
    kw = dict(cfg=cfg, backbone="ViT-L/14", r=16, sd_seed=17, B=4, C=6, max_len=20, fused=True)
    a = _setup(dev, **kw)
    la, _, _ = _step(a)
    ref = a.tr.flat.grads.clone()
    rmax = ref.abs().max().item()
    assert torch.isfinite(ref).all() and rmax > 1e-5
    b = _setup(dev, loss_scale=2.0 ** 12, **kw)
    b.model.engine.precision = "fp16"
    lb, _, _ = _step(b)
    got = b.tr.flat.grads * 2.0 ** -12
    err = (got - ref).abs().max().item()
    print(f"fp16 storage mode, loss_scale 2^12: max grad error {err:.3e} of largest fp32 entry {rmax:.3e}; "
          f"loss {lb.item():.6f} vs fp32 {la.item():.6f}")
    assert torch.isfinite(b.tr.flat.grads).all() and (b.tr.skipped_steps, b.tr.optimizer_steps) == (0, 1)
    assert err < 3e-2 * rmax
