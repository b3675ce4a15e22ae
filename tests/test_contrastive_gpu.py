"""The contrastive objective on the MI355X: clipfs_contrastive_objective against the fp64 reference of contrastive_ref.py,
its exactness properties (bitwise run to run, accumulate = old + fresh, a power-of-two loss scale, optional outputs, guard
rows), ops.clip_loss, and LoRATrainer.step_pairs against fp64 autograd on the oracle, on two data-parallel ranks and
without host synchronisation.

Tolerances are 4 x the worst error measured on an MI355X (the project's convention, DESIGN.md sections 22-24: the factor
absorbs run-to-run-independent differences in summation order across shapes while still catching a wrong term).  Every
test prints its figures before it asserts.

    quantity                                                        worst measured   bound
    loss_sum (w = 1/R; kernel cases and clip_loss), absolute        8.52e-7          3.5e-6
    loss_rows, absolute                                             1.82e-5          7.3e-5
    kernel dq / dk, share of the reference's largest entry          2.25e-5          9.0e-5
    clip_loss gradients, share of the largest entry                 1.16e-5          4.7e-5
    step_pairs loss against the fp64 oracle, absolute               1.10e-6          4.4e-6
    step_pairs adapter gradients (the whole flat buffer), share     4.27e-6          1.8e-5
    two ranks against one process: flat gradient, share             2.05e-6          8.2e-6
    two ranks against one process: summed loss, absolute            0 (equal)        1e-6

The last bound is not 4 x a measurement (that would be 0): the two ranks add the same fp32 row losses in another order than
one process does, which may move a loss of ~2.8 by a few units in its last place (2.4e-7); 1e-6 is four of them.  For
orientation, a torch fp32 CPU evaluation of the kernel cases is within 7.5e-7 on the loss and 3.9e-6 on the gradients.
The loss_rows and dq / dk figures are those of (4081, 40, 600, groups) at s = 100, measured on the kernels as they stood
before logits_tile.h (the older cases gave 1.51e-5 and 1.77e-5).
"""
import os
import socket
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from contrastive_ref import CASES, contrastive_case, contrastive_inputs, contrastive_ref, symmetric_loss

pytestmark = pytest.mark.gpu

BOUND_LOSS = 3.5e-6
BOUND_ROWS = 7.3e-5
BOUND_GRAD = 9.0e-5
BOUND_CLIP = 4.7e-5
BOUND_TLOSS = 4.4e-6
BOUND_TGRAD = 1.8e-5
BOUND_DP_LOSS = 1e-6
BOUND_DP_GRAD = 8.2e-6


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _run(dev, q, k, qg, kg, s, w, **kw):
    from clipfs import ops
    return ops.contrastive_objective(q.to(dev), k.to(dev), qg.to(dev), kg.to(dev), s, w, **kw)


def _share(got, want, floor):
    """Largest error as a share of the reference's largest entry (``floor``: the bound w s of an entry, for a reference that
    is zero but for fp64 rounding: one key, or identical keys, whose terms cancel)."""
    scale = want.abs().max().item()
    return (got.detach().double().cpu() - want).abs().max().item() / (scale if scale > 1e-9 * floor else floor)


def _check(dev, q, k, qg, kg, s, w, ref, tag, want_correct=None):
    loss, rows, correct, dq, dk = _run(dev, q, k, qg, kg, s, w)
    e_loss = abs(loss.item() - float(ref["loss"]))
    e_rows = (rows.double().cpu() - ref["loss_rows"]).abs().max().item()
    e_dq, e_dk = _share(dq, ref["dq"], abs(w * s)), _share(dk, ref["dk"], abs(w * s))
    want_correct = ref["correct"] if want_correct is None else want_correct
    print(f"{tag}: loss {e_loss:.3e} rows {e_rows:.3e} dq {e_dq:.3e} dk {e_dk:.3e} correct {correct.item()} / {want_correct}")
    assert e_loss <= BOUND_LOSS and e_rows <= BOUND_ROWS
    assert e_dq <= BOUND_GRAD and e_dk <= BOUND_GRAD
    assert correct.item() == want_correct
    return loss, rows, correct, dq, dk


# ------------------------------------------------------------------------------------------- 1. kernel against the reference
@pytest.mark.parametrize("R,N,d,kind", CASES)
@pytest.mark.parametrize("s", [100.0, 1.0])
def test_kernel_against_reference(dev, R, N, d, kind, s):
    q, k, qg, kg, ref = contrastive_case(R, N, d, kind, s)
    _check(dev, q, k, qg, kg, s, 1.0 / R, ref, f"({R}, {N}, {d}, {kind}) s={s:g}")


# ------------------------------------------------------------------------------------------- 2. edge cases
def test_identical_keys_give_a_uniform_softmax_and_index_zero(dev):
    R, N, d = 40, 70, 64
    q, k, _, _ = contrastive_inputs(R, N, d, "groups")
    k = k[3:4].repeat(N, 1).contiguous()
    qg, kg = (torch.arange(R) % 3).to(torch.int32), ((torch.arange(N) + 1) % 3).to(torch.int32)
    ref = contrastive_ref(q, k, qg, kg, 100.0, 1.0 / R)
    # every row's arg-max is key 0 (the fp64 matmul of the reference does not promise bitwise equal columns)
    loss, rows, correct, dq, dk = _check(dev, q, k, qg, kg, 100.0, 1.0 / R, ref, "identical keys", int((qg == kg[0]).sum()))
    assert (rows.cpu() - float(np.log(N))).abs().max().item() <= BOUND_ROWS  # lse - z = log N whatever the positives


def test_no_row_has_a_positive(dev):
    q, k, _, _ = contrastive_inputs(37, 83, 192, "groups")
    qg, kg = torch.full((37,), 5, dtype=torch.int32), torch.full((83,), 7, dtype=torch.int32)
    kg[::9] = -1
    loss, rows, correct, dq, dk = _run(dev, q, k, qg, kg, 100.0, 1.0)
    print("no positives:", loss.item(), rows.abs().max().item(), correct.item(), dq.abs().max().item(), dk.abs().max().item())
    assert loss.item() == 0 and rows.abs().max().item() == 0 and correct.item() == 0
    assert dq.abs().max().item() == 0 and dk.abs().max().item() == 0
    old = torch.randn(37, 192, device=dev)
    _, _, _, dq2, _ = _run(dev, q, k, qg, kg, 100.0, 1.0, dq=old.clone(), want_dk=False)
    assert torch.equal(dq2, old)


@pytest.mark.parametrize("side", ["keys", "queries"])
def test_one_side_masked_except_one_row(dev, side):
    R, N, d = 33, 65, 64
    q, k, qg, kg = contrastive_inputs(R, N, d, "groups")
    if side == "keys":
        keep = int((kg >= 0).nonzero()[5])
        g = int(kg[keep])
        kg = torch.full_like(kg, -1)
        kg[keep] = g
        qg[:4] = g  # at least four rows whose one positive is the one key: loss 0
    else:
        keep = int((qg >= 0).nonzero()[5])
        g = int(qg[keep])
        qg = torch.full_like(qg, -1)
        qg[keep] = g
        kg[:4] = g
    ref = contrastive_ref(q, k, qg, kg, 100.0, 1.0 / R)
    loss, rows, correct, dq, dk = _check(dev, q, k, qg, kg, 100.0, 1.0 / R, ref, f"all {side} masked but one")
    if side == "keys":
        dead = torch.arange(N) != keep
        assert dk.cpu()[dead].abs().max().item() == 0 and correct.item() == int((qg == g).sum())
    else:
        dead = torch.arange(R) != keep
        assert dq.cpu()[dead].abs().max().item() == 0 and rows.cpu()[dead].abs().max().item() == 0


# ------------------------------------------------------------------------------------------- 3.-6. exactness
def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("R,N,d,kind", [(256, 403, 512, "groups"), (96, 1100, 1024, "groups")])
def test_two_runs_are_bitwise_equal(dev, R, N, d, kind):
    q, k, qg, kg = contrastive_inputs(R, N, d, kind)
    assert _same(_run(dev, q, k, qg, kg, 100.0, 1.0 / R), _run(dev, q, k, qg, kg, 100.0, 1.0 / R))


@pytest.mark.parametrize("R,N,d,kind", [(33, 65, 64, "groups"), (256, 256, 512, "paired")])
def test_accumulate_is_bitwise_old_plus_fresh(dev, R, N, d, kind):
    q, k, qg, kg = contrastive_inputs(R, N, d, kind)
    fresh = _run(dev, q, k, qg, kg, 100.0, 1.0 / R)
    g = torch.Generator().manual_seed(3)
    old_q, old_k = torch.randn(R, d, generator=g).to(dev), torch.randn(N, d, generator=g).to(dev)
    acc = _run(dev, q, k, qg, kg, 100.0, 1.0 / R, dq=old_q.clone(), dk=old_k.clone())
    assert _same(acc[:3], fresh[:3])
    assert torch.equal(acc[3], old_q + fresh[3]) and torch.equal(acc[4], old_k + fresh[4])
    # ... and a passed buffer is overwritten with accumulate=False
    over = _run(dev, q, k, qg, kg, 100.0, 1.0 / R, dq=old_q.clone(), dk=old_k.clone(), accumulate=(False, True))
    assert torch.equal(over[3], fresh[3]) and torch.equal(over[4], acc[4])


def test_loss_scale_record_multiplies_the_gradients_only(dev):
    from clipfs import ops
    q, k, qg, kg = contrastive_inputs(33, 65, 64, "groups")
    plain = _run(dev, q, k, qg, kg, 100.0, 1.0 / 33)
    state = ops.new_scaler_state(4096.0, dev)
    keep = state.clone()
    scaled = _run(dev, q, k, qg, kg, 100.0, 1.0 / 33, scale_state=state)
    assert _same(scaled[:3], plain[:3])
    assert torch.equal(scaled[3], plain[3] * 4096.0) and torch.equal(scaled[4], plain[4] * 4096.0)
    assert plain[3].abs().max().item() > 0 and torch.equal(state, keep)


def test_an_absent_gradient_leaves_the_other_unchanged(dev):
    q, k, qg, kg = contrastive_inputs(37, 83, 192, "groups")
    both = _run(dev, q, k, qg, kg, 100.0, 1.0 / 37)
    only_k = _run(dev, q, k, qg, kg, 100.0, 1.0 / 37, want_dq=False)
    only_q = _run(dev, q, k, qg, kg, 100.0, 1.0 / 37, want_dk=False)
    none = _run(dev, q, k, qg, kg, 100.0, 1.0 / 37, want_dq=False, want_dk=False)
    assert only_k[3] is None and only_q[4] is None and none[3] is None and none[4] is None
    assert _same(only_k[:3], both[:3]) and _same(only_q[:3], both[:3]) and _same(none[:3], both[:3])
    assert torch.equal(only_k[4], both[4]) and torch.equal(only_q[3], both[3])


# ------------------------------------------------------------------------------------------- 7. extents
@pytest.mark.parametrize("R,N,d", [(37, 83, 192), (33, 300, 64), (1, 1, 64)])
def test_guard_rows_and_the_tail_of_work_are_untouched(dev, R, N, d):
    from clipfs import _lib, ops
    q, k, qg, kg = contrastive_inputs(R, N, d, "groups" if R > 1 else "paired")
    q, k, qg, kg = q.to(dev), k.to(dev), qg.to(dev), kg.to(dev)
    wf = ops.contrastive_plan("stats", R, N, d)["work_floats"]
    mark = 7.25
    work = torch.full((wf + 64,), mark, device=dev)
    rows = torch.full((R + 8,), mark, device=dev)
    dq = torch.full((R + 2, d), mark, device=dev)
    dk = torch.full((N + 2, d), mark, device=dev)
    lsum = torch.full((4,), mark, device=dev)
    cor = torch.full((4,), 77, device=dev, dtype=torch.int32)
    rc = _lib.load().clipfs_contrastive_objective(q.data_ptr(), k.data_ptr(), qg.data_ptr(), kg.data_ptr(), 100.0, 1.0 / R, None,
                                                  rows.data_ptr() + 16, lsum.data_ptr(), cor.data_ptr(), dq[1:].data_ptr(), 0,
                                                  dk[1:].data_ptr(), 0, work.data_ptr(), R, N, d,
                                                  torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.load().clipfs_last_error()
    assert (work[wf:] == mark).all() and (rows[:4] == mark).all() and (rows[4 + R:] == mark).all()
    assert (dq[0] == mark).all() and (dq[R + 1] == mark).all() and (dk[0] == mark).all() and (dk[N + 1] == mark).all()
    assert (lsum[1:] == mark).all() and (cor[1:] == 77).all()
    want = ops.contrastive_objective(q, k, qg, kg, 100.0, 1.0 / R)
    assert torch.equal(rows[4:4 + R], want[1]) and torch.equal(dq[1:R + 1], want[3]) and torch.equal(dk[1:N + 1], want[4])
    assert lsum[0].item() == want[0].item() and cor[0].item() == want[2].item()


# ------------------------------------------------------------------------------------------- 8. the autograd Function
@pytest.mark.parametrize("B,M,d,kind", [(32, 32, 64, "paired"), (33, 65, 64, "groups"), (300, 40, 128, "groups")])
def test_clip_loss_gradients(dev, B, M, d, kind):
    from clipfs import ops
    q, k, qg, kg = contrastive_inputs(B, M, d, kind)
    img, txt = q.to(dev).requires_grad_(), k.to(dev).requires_grad_()
    groups = (None, None) if kind == "paired" else (qg.to(dev), kg.to(dev))
    loss = ops.clip_loss(img, txt, *groups)
    (3.0 * loss).backward()
    a = contrastive_ref(q, k, qg, kg, 100.0, 0.5 / B)
    b = contrastive_ref(k, q, kg, qg, 100.0, 0.5 / M)
    e_loss = abs(loss.item() - float(a["loss"] + b["loss"]))
    e_i, e_t = _share(img.grad, 3.0 * (a["dq"] + b["dk"]), 1.0), _share(txt.grad, 3.0 * (a["dk"] + b["dq"]), 1.0)
    print(f"clip_loss ({B}, {M}, {d}, {kind}): loss {e_loss:.3e} dimg {e_i:.3e} dtxt {e_t:.3e}")
    assert e_loss <= BOUND_LOSS and e_i <= BOUND_CLIP and e_t <= BOUND_CLIP
    # a side that needs no gradient gets none, the other side's is bitwise the same
    img2 = q.to(dev).requires_grad_()
    (3.0 * ops.clip_loss(img2, k.to(dev), *groups)).backward()
    assert torch.equal(img2.grad, img.grad)


# ------------------------------------------------------------------------------------------- 9. the trainer against the oracle
def _positions(cfg):
    return list(range(cfg.transformer_layers)), list(range(cfg.vision_layers))


def _model(dev, monkey, p=0.0, encoder="both"):
    """The suite's small test model with rank-4 q/k/v adapters (the pattern of test_engine_gpu.py)."""
    import lora_train_vlp as L
    from clipfs import synth
    from jclip.model import build_model
    cfg = synth.SMALL
    sd = synth.synth_state_dict(cfg, seed=11, perturb=True)
    model = build_model(sd, device=dev)
    args = types.SimpleNamespace(encoder=encoder, position="all", backbone="small", params=["q", "k", "v"], r=4, alpha=1,
                                 dropout_rate=p)
    tb, vb = _positions(cfg)
    monkey.setitem(L.INDEX_POSITIONS_TEXT, "all", tb)
    monkey.setitem(L.INDEX_POSITIONS_VISION.setdefault("small", {}), "all", vb)
    layers = L.apply_lora(args, model)
    lw = synth.synth_lora(cfg, 4, seed=5)
    names = {"q": "q_proj", "k": "k_proj", "v": "v_proj"}
    first = len(tb) if encoder == "vision" else 0
    with torch.no_grad():
        for i, layer in enumerate(layers):
            for pr in "qkv":
                mod = getattr(layer, names[pr])
                mod.w_lora_A.copy_(torch.from_numpy(lw[f"layer_{first + i}"][names[pr]]["w_lora_A"]))
                mod.w_lora_B.copy_(torch.from_numpy(lw[f"layer_{first + i}"][names[pr]]["w_lora_B"]))
    L.mark_only_lora_as_trainable(model)
    return L, cfg, sd, model, layers, lw


def _oracle_lora(lw, cfg):
    tb, vb = _positions(cfg)
    conv = lambda dd: {p: {k: torch.from_numpy(v).double().requires_grad_() for k, v in ab.items()} for p, ab in dd.items()}
    return ({b: conv(lw[f"layer_{i}"]) for i, b in enumerate(tb)},
            {b: conv(lw[f"layer_{len(tb) + i}"]) for i, b in enumerate(vb)})


def _batch(cfg, kind, B=6, M=4):
    from clipfs import synth
    if kind == "paired":
        M = B
    img = synth.synth_images(B, cfg.image_resolution, seed=3)
    cap = synth.synth_captions(M, cfg.context_length, cfg.vocab_size, seed=4, max_len=12)
    if kind == "paired":
        return img, cap, None, None
    return img, cap, synth.synth_labels(B, M, seed=2).to(torch.int32), torch.arange(M, dtype=torch.int32)


def _oracle_step(cfg, sd, lw, img, cap, ig, cg, seed, p, encoder="both"):
    """loss and the adapter gradients (apply_lora order) of the pair objective by fp64 autograd on the oracle."""
    from oracle import clip_oracle as O
    sd64 = {k: v.double() for k, v in sd.items()}
    tl, vl = _oracle_lora(lw, cfg)
    B, M = img.shape[0], cap.shape[0]
    names = ("q_proj", "k_proj", "v_proj")

    def drops(width, seq, n, layers_n, stream0):
        if p == 0:
            return None
        out = {}
        for l in range(layers_n):
            dd = {}
            for s_, nm in enumerate(names):
                keep = O.dropout_keep_mask(seed, stream0 + 4 * l + s_, n * seq, width, p)
                dd[nm] = (torch.from_numpy(keep).double() / (1 - p)).reshape(n, seq, width).permute(1, 0, 2)
            out[l] = dd
        return out

    td = drops(cfg.transformer_width, cfg.context_length, M, cfg.transformer_layers, 0)
    vd = drops(cfg.vision_width, cfg.vision_tokens, B, cfg.vision_layers, 1000)
    sc = O.lora_scaling(1, 4)
    use_t, use_v = encoder in ("both", "text"), encoder in ("both", "vision")
    emb = O.encode_text(sd64, cap, tl if use_t else None, sc, drops=td if use_t else None)
    txt = O.class_text_features(emb, list(range(M)), M).t()
    feat = O.l2_normalize(O.encode_image(sd64, img.double(), vl if use_v else None, sc, drops=vd if use_v else None))
    if ig is None:
        ig = cg = torch.arange(B, dtype=torch.int32)
    loss = symmetric_loss(feat, txt, ig, cg)
    loss.backward()
    blocks = (list(tl.values()) if use_t else []) + (list(vl.values()) if use_v else [])
    return loss.item(), blocks, (feat.detach(), txt.detach())


def _grad_error(layers, blocks, flat):
    """Worst adapter-gradient error as a share of the largest reference entry; the pairs must cover the flat buffer."""
    gmax = max(t.grad.abs().max().item() for blk in blocks for ab in blk.values() for t in ab.values())
    worst, covered = 0.0, 0
    for layer, blk in zip(layers, blocks):
        pairs = dict((id(prm), g) for prm, g in layer.trainable_pairs())
        for nm in ("q_proj", "k_proj", "v_proj"):
            mod = getattr(layer, nm)
            for w_, prm in (("w_lora_A", mod.w_lora_A), ("w_lora_B", mod.w_lora_B)):
                got = pairs[id(prm)]
                covered += got.numel()
                worst = max(worst, (got.double().cpu() - blk[nm][w_].grad).abs().max().item())
    assert covered == flat.numel, (covered, flat.numel)
    assert gmax > 1e-4
    return worst / gmax


@pytest.mark.parametrize("kind", ["paired", "groups"])
@pytest.mark.parametrize("p", [0.0, 0.25])
def test_step_pairs_against_oracle(dev, monkeypatch, kind, p):
    from clipfs.engine import _mix_seed
    L, cfg, sd, model, layers, lw = _model(dev, monkeypatch, p)
    img, cap, ig, cg = _batch(cfg, kind)
    model.train()
    tr = L.LoRATrainer(model)
    tr.flat.zero_grad()
    dg = lambda t: None if t is None else t.to(dev)
    loss, c_it, c_ti = tr.forward_backward_pairs(img.to(dev), cap.to(dev), dg(ig), dg(cg))
    seed = _mix_seed(model.engine.seed_base, model.engine.step)
    want, blocks, (feat, txt) = _oracle_step(cfg, sd, lw, img, cap, ig, cg, seed, p)
    e_loss, e_grad = abs(loss.item() - want), _grad_error(layers, blocks, tr.flat)
    print(f"step_pairs {kind} p={p}: loss {loss.item():.6f} err {e_loss:.3e} grad {e_grad:.3e} hits {c_it.item()} {c_ti.item()}")
    assert tr.last_plan["vision"] is not None and tr.last_plan["text"] is not None
    assert e_loss <= BOUND_TLOSS and e_grad <= BOUND_TGRAD
    B, M = img.shape[0], cap.shape[0]
    g_i, g_c = (torch.arange(B), torch.arange(M)) if ig is None else (ig.long(), cg.long())
    z = 100.0 * feat @ txt.t()
    assert c_it.item() == int((g_c[z.argmax(1)] == g_i).sum()) and c_ti.item() == int((g_i[z.argmax(0)] == g_c).sum())


def test_step_pairs_text_encoder_only(dev, monkeypatch):
    L, cfg, sd, model, layers, lw = _model(dev, monkeypatch, 0.0, encoder="text")
    img, cap, ig, cg = _batch(cfg, "groups")
    model.eval()
    tr = L.LoRATrainer(model)
    tr.flat.zero_grad()
    calls = []
    real = model.engine.vit_backward
    monkeypatch.setattr(model.engine, "vit_backward", lambda *a, **k: calls.append(1) or real(*a, **k))
    loss, _, _ = tr.forward_backward_pairs(img.to(dev), cap.to(dev), ig.to(dev), cg.to(dev))
    want, blocks, _ = _oracle_step(cfg, sd, lw, img, cap, ig, cg, 0, 0.0, encoder="text")
    e_loss, e_grad = abs(loss.item() - want), _grad_error(layers, blocks, tr.flat)
    print(f"step_pairs text only: loss err {e_loss:.3e} grad {e_grad:.3e}")
    assert tr.last_plan["vision"] is None and tr.last_plan["text"] is not None and not calls
    assert e_loss <= BOUND_TLOSS and e_grad <= BOUND_TGRAD


def test_three_scaled_steps_end_bitwise_on_the_unscaled_parameters(dev, monkeypatch):
    out = []
    for scale in (None, 2.0 ** 12):
        L, cfg, sd, model, layers, lw = _model(dev, monkeypatch, 0.25)
        img, cap, ig, cg = _batch(cfg, "groups")
        model.train()
        tr = L.LoRATrainer(model, lr=1e-3, loss_scale=scale)
        losses = [tr.step_pairs(img.to(dev), cap.to(dev), ig.to(dev), cg.to(dev))[0].item() for _ in range(3)]
        out.append((losses, tr.flat.params.clone()))
        assert tr.skipped_steps == 0 and tr.optimizer_steps == 3
    assert out[0][0] == out[1][0] and out[0][0][2] != out[0][0][0]
    assert torch.equal(out[0][1], out[1][1])


def test_pairs_refusals(dev, monkeypatch):
    L, cfg, sd, model, layers, lw = _model(dev, monkeypatch)
    img, cap, ig, cg = _batch(cfg, "groups")
    tr = L.LoRATrainer(model)
    with pytest.raises(ValueError, match="6 images, 4 captions"):
        tr.forward_backward_pairs(img.to(dev), cap.to(dev))
    with pytest.raises(ValueError, match="both image_groups and caption_groups"):
        tr.forward_backward_pairs(img.to(dev), cap.to(dev), ig.to(dev))


# ------------------------------------------------------------------------------------------- 10. two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _Monkey:
    """monkeypatch.setitem for a spawned rank (no fixture there); nothing is restored: the process ends."""

    @staticmethod
    def setitem(d, k, v):
        d[k] = v


DP_B, DP_M = 7, 5


def _dp_step(dev, monkey, rank=0, world=1, shard_text=True):
    from clipfs import dist as D
    L, cfg, sd, model, layers, lw = _model(dev, monkey)
    img, cap, ig, cg = _batch(cfg, "groups", DP_B, DP_M)
    model.eval()
    tr = L.LoRATrainer(model, shard_text=shard_text)
    b0, b1 = D.block_bounds(DP_B, rank, world)
    c0, c1 = D.block_bounds(DP_M, rank, world)
    tr.flat.zero_grad()
    out = tr.forward_backward_pairs(img[b0:b1].to(dev), cap[c0:c1].to(dev), ig[b0:b1].to(dev), cg[c0:c1].to(dev), DP_B, DP_M,
                                    row_offset=b0, caption_offset=c0)
    return tr, out


def _pairs_rank(rank, world, port, out_dir):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for path in (os.path.join(root, "jittor-clip-fewshot_amd"), root, os.path.join(root, "tests")):
        if path not in sys.path:
            sys.path.insert(0, path)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    from clipfs import dist as D
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda:0")
    tr, (loss, c_it, c_ti) = _dp_step(dev, _Monkey, rank, world)
    assert (tr.rank, tr.world) == (rank, world) and tr.collectives_per_step == 6
    tr.optimizer_step()
    total = torch.cat([loss, c_it.float(), c_ti.float()])
    D.allreduce_sum_(total)
    torch.cuda.synchronize()
    if rank == 0:
        np.savez(os.path.join(out_dir, "pairs.npz"), grads=tr.flat.grads.cpu().numpy(), total=total.cpu().numpy())
    refused = False
    try:
        _dp_step(dev, _Monkey, rank, world, shard_text=False)
    except ValueError as e:
        refused = "shard_text=False" in str(e)
    assert refused
    dist.destroy_process_group()


def test_two_ranks_match_one_process(dev, monkeypatch, tmp_path):
    """B_g = 7 and M_g = 5 on two ranks: blocks of 4 + 3 images and 3 + 2 captions, a padding row on either side."""
    tr, (loss, c_it, c_ti) = _dp_step(dev, monkeypatch)
    want_g = tr.flat.grads.cpu().numpy()
    mp.spawn(_pairs_rank, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    z = np.load(os.path.join(str(tmp_path), "pairs.npz"))
    scale = np.abs(want_g).max()
    e_loss, e_grad = abs(float(z["total"][0]) - loss.item()), np.abs(z["grads"] - want_g).max() / scale
    print(f"two ranks: loss {loss.item():.6f} err {e_loss:.3e} grad {e_grad:.3e} hits {z['total'][1:]} / {c_it.item()} {c_ti.item()}")
    assert scale > 1e-5
    assert e_loss <= BOUND_DP_LOSS and e_grad <= BOUND_DP_GRAD
    assert (int(z["total"][1]), int(z["total"][2])) == (c_it.item(), c_ti.item())


# ------------------------------------------------------------------------------------------- 11. retrieval
def test_evaluate_retrieval(dev, monkeypatch):
    from clipfs import synth
    L, cfg, sd, model, layers, lw = _model(dev, monkeypatch)
    model.eval()
    B, M = 12, 9
    img = synth.synth_images(B, cfg.image_resolution, seed=3).to(dev)
    cap = synth.synth_captions(M, cfg.context_length, cfg.vocab_size, seed=4, max_len=12).to(dev)
    ig, cg = synth.synth_labels(B, 4, seed=2), synth.synth_labels(M, 4, seed=6)
    got = L.evaluate_retrieval(model, img, cap, ig, cg, ks=(1, 5, 10))
    with torch.no_grad():
        fi, ft = model.encode_image(img).double().cpu(), model.encode_text(cap).double().cpu()
    fi, ft = fi / fi.norm(dim=1, keepdim=True), ft / ft.norm(dim=1, keepdim=True)
    z = fi @ ft.t()
    want = {}
    for name, zz, qg, kg in (("i2t", z, ig, cg), ("t2i", z.t(), cg, ig)):
        order = zz.argsort(dim=1, descending=True, stable=True)
        want[name] = {k: int((kg[order[:, :k]] == qg[:, None]).any(1).sum()) / zz.shape[0] for k in (1, 5, 10)}
    print("retrieval:", got, want)
    assert got == want
    assert want["i2t"][1] <= want["i2t"][5] <= want["i2t"][10] and 0 < want["i2t"][10] <= 1
    paired = L.evaluate_retrieval(model, img[:M], cap, ks=(1, 3))
    assert set(paired) == {"i2t", "t2i"} and set(paired["i2t"]) == {1, 3}
    with pytest.raises(ValueError, match="12 images, 9 captions"):
        L.evaluate_retrieval(model, img, cap)


# ------------------------------------------------------------------------------------------- 12. no host synchronisation
def test_step_pairs_does_not_synchronise(dev, monkeypatch):
    L, cfg, sd, model, layers, lw = _model(dev, monkeypatch, 0.25)
    img, cap, ig, cg = (t.to(dev) for t in _batch(cfg, "groups"))
    model.train()
    tr = L.LoRATrainer(model, loss_scale=2.0 ** 12, max_grad_norm=1.0)
    tr.step_pairs(img, cap, ig, cg)  # warm-up: the text tower's row plan of this caption table, the workspaces
    tr.step_pairs(img[:4].contiguous(), cap, None, None)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, c_it, c_ti = tr.step_pairs(img, cap, ig, cg)
        tr.step_pairs(img[:4].contiguous(), cap, None, None)  # pairs: the group vectors are made on the device
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(loss).all() and 0 <= c_it.item() <= 6 and 0 <= c_ti.item() <= 4
