"""The sigmoid (SigLIP) objective on the MI355X: clipfs_sigmoid_objective against the fp64 reference of sigmoid_ref.py in
three regimes of (t, b), its edge cases and exactness properties (bitwise run to run, accumulate = old + fresh, a
power-of-two loss scale, optional outputs, poisoned outputs, guard rows), ops.siglip_loss, and LoRATrainer.step_pairs
under LoRAPairTrainer(pair_loss="sigmoid") against fp64 autograd on the oracle, on two data-parallel ranks and without host
synchronisation.  The test model, the batches and the oracle step are those of test_contrastive_gpu.py.

Kernel bounds are not constants: per quantity and regime, 16 x the worst error of the fp32 yardstick (the reference's own
expressions evaluated in torch fp32 on the CPU) over the case table, and at least 1e-6.  16 = 4 x the project's usual
4 x margin; 4 is what the InfoNCE kernels measured against the same kind of yardstick.  The
yardstick is computed at run time, never from the kernels' output.  Error denominators: the reference value for loss_sum
and the row losses (all terms >= 0), the reference's largest entry for dq / dk, t sum |G a| and sum |G| for dhead (and
their per-row forms for rows 1 and 2 of row_stats).  Every test prints its figures before it asserts.

Trainer bounds are the InfoNCE trainer's (test_contrastive_gpu.py: BOUND_TGRAD, BOUND_DP_GRAD as shares of the largest
entry; BOUND_TLOSS and the data-parallel loss bound as they stand there for a loss of O(1), here times max(1, loss)): what
they absorb is the towers' fp32 error and the towers' kernel choice per batch size, which do not depend on the
objective; the objective's own error is bounded by the kernel tests above.  The head's two gradient entries are measured
against their cancellation-free scales, like dhead.
"""
import functools
import math
import os
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import poison
import test_contrastive_gpu as TC
from contrastive_ref import contrastive_inputs
from sigmoid_ref import CASES, REGIMES, head_of, sigmoid_case, sigmoid_loss, sigmoid_ref

pytestmark = pytest.mark.gpu

FACTOR, FLOOR = 16.0, 1e-6
QUANTITIES = ("loss", "rows", "rows_g", "rows_ga", "dq", "dk", "dhead_t", "dhead_b")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _run(dev, q, k, qg, kg, head, w, **kw):
    from clipfs import ops
    for name in ("dq", "dk", "dhead", "scale_state"):
        if kw.get(name) is not None:
            kw[name] = kw[name].to(dev)
    return ops.sigmoid_objective(q.to(dev), k.to(dev), qg.to(dev), kg.to(dev), head.to(dev), w, **kw)


def _as_dict(out):
    loss, rows, correct, dq, dk, dhead = out
    return dict(loss=loss[0], rows=rows, dq=dq, dk=dk, dhead=dhead, correct=int(correct.item()),
                best=rows[3].view(torch.int32).long().cpu())


def _ratio(err, den):
    """max of err / den over the entries whose denominator is not zero (0 where there is none)."""
    m = den > 0
    return float((err[m] / den[m]).max()) if bool(m.any()) else 0.0


def _errors(got, ref):
    """The eight error figures of ``got`` (kernel outputs or the fp32 yardstick) against the fp64 reference ``ref``."""
    f = lambda x: x.detach().double().cpu()
    top = lambda x: x.abs().max()
    rows, want = f(got["rows"]), ref["rows"]
    return dict(
        loss=float((f(got["loss"]) - ref["loss"]).abs() / ref["loss"]) if float(ref["loss"]) > 0 else float(f(got["loss"]).abs()),
        rows=_ratio((rows[0] - want[0]).abs(), want[0]),
        rows_g=_ratio((rows[1] - want[1]).abs(), ref["rows_scale"][0]),
        rows_ga=_ratio((rows[2] - want[2]).abs(), ref["rows_scale"][1]),
        dq=float(top(f(got["dq"]) - ref["dq"]) / top(ref["dq"])),
        dk=float(top(f(got["dk"]) - ref["dk"]) / top(ref["dk"])),
        dhead_t=float((f(got["dhead"])[0] - ref["dhead"][0]).abs() / ref["scale_t"]),
        dhead_b=float((f(got["dhead"])[1] - ref["dhead"][1]).abs() / ref["scale_b"]))


@functools.lru_cache(maxsize=None)
def _bounds(regime):
    """{quantity: bound} of one regime: FACTOR x the yardstick's worst error over the case table, at least FLOOR."""
    worst = dict.fromkeys(QUANTITIES, 0.0)
    for case in CASES:
        *_, ref, yard = sigmoid_case(*case, regime)
        for name, e in _errors(yard, ref).items():
            worst[name] = max(worst[name], e)
    return {name: max(FACTOR * e, FLOOR) for name, e in worst.items()}


def _check(got, ref, regime, tag):
    err, bound = _errors(got, ref), _bounds(regime)
    print(f"{tag} [{regime}]: " + " ".join(f"{n} {err[n]:.2e}/{bound[n]:.2e}" for n in QUANTITIES)
          + f" correct {got['correct']} / {ref['correct']}")
    dead = ref["rows"][3] < 0
    assert bool((got["rows"][:3].cpu()[:, dead] == 0).all()), "a dead query's row statistics are exactly 0"
    assert torch.equal(got["best"], ref["best"]) and got["correct"] == ref["correct"]
    for name in QUANTITIES:
        assert err[name] <= bound[name], (tag, regime, name, err[name], bound[name])
    return err


# ------------------------------------------------------------------------------------------- 1. kernel against the reference
@pytest.mark.parametrize("R,N,d,kind", CASES)
@pytest.mark.parametrize("regime", list(REGIMES))
def test_kernel_against_reference(dev, R, N, d, kind, regime):
    q, k, qg, kg, head, ref, _ = sigmoid_case(R, N, d, kind, regime)
    _check(_as_dict(_run(dev, q, k, qg, kg, head, 1.0 / R)), ref, regime, f"({R}, {N}, {d}, {kind})")


# ------------------------------------------------------------------------------------------- 2. edge cases
MIXED = head_of(*REGIMES["mixed"])


def test_every_key_masked(dev):
    R, N, d = 37, 83, 192
    q, k, qg, _ = contrastive_inputs(R, N, d, "groups")
    kg = torch.full((N,), -1, dtype=torch.int32)
    old = torch.full((2,), 3.0)
    loss, rows, correct, dq, dk, dhead = _run(dev, q, k, qg, kg, MIXED, 1.0, dhead=old.clone())
    print("every key masked:", loss.item(), correct.item(), dq.abs().max().item(), dk.abs().max().item(), dhead.tolist())
    assert loss.item() == 0 and correct.item() == 0 and bool((rows[:3] == 0).all())
    assert bool((rows[3].view(torch.int32) == -1).all())
    assert dq.abs().max().item() == 0 and dk.abs().max().item() == 0 and torch.equal(dhead.cpu(), old)


def test_every_query_masked_but_one(dev):
    R, N, d = 33, 65, 64
    q, k, qg, kg = contrastive_inputs(R, N, d, "groups")
    keep = int((qg >= 0).nonzero()[5])
    g = int(qg[keep])
    qg = torch.full_like(qg, -1)
    qg[keep] = g
    kg[:4] = g
    ref = sigmoid_ref(q, k, qg, kg, MIXED, 1.0 / R)
    got = _as_dict(_run(dev, q, k, qg, kg, MIXED, 1.0 / R))
    _check(got, ref, "mixed", "all queries masked but one")
    dead = torch.arange(R) != keep
    assert got["dq"].cpu()[dead].abs().max().item() == 0 and bool((got["best"][dead] == -1).all())
    assert got["dk"].cpu()[kg < 0].abs().max().item() == 0


def test_no_positive_anywhere(dev):
    R, N, d = 37, 83, 192
    q, k, _, _ = contrastive_inputs(R, N, d, "groups")
    qg, kg = torch.full((R,), 5, dtype=torch.int32), torch.full((N,), 7, dtype=torch.int32)
    kg[::9] = -1
    ref = sigmoid_ref(q, k, qg, kg, MIXED, 1.0 / R)
    got = _as_dict(_run(dev, q, k, qg, kg, MIXED, 1.0 / R))
    _check(got, ref, "mixed", "no positive")  # a row without a positive still pays its negative terms
    assert got["loss"].item() > 0 and got["correct"] == 0 and bool((got["rows"][0] > 0).all())
    assert got["dq"].abs().max().item() > 0


def test_identical_keys_give_index_zero(dev):
    R, N, d = 40, 70, 64
    q, k, _, _ = contrastive_inputs(R, N, d, "groups")
    k = k[3:4].repeat(N, 1).contiguous()
    qg, kg = (torch.arange(R) % 3).to(torch.int32), ((torch.arange(N) + 1) % 3).to(torch.int32)
    got = _as_dict(_run(dev, q, k, qg, kg, MIXED, 1.0 / R))
    print("identical keys: best", got["best"].unique().tolist(), "correct", got["correct"])
    assert bool((got["best"] == 0).all()) and got["correct"] == int((qg == kg[0]).sum())


# ------------------------------------------------------------------------------------------- 3. exactness
def _same(a, b):
    return all(poison.same_bits(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("R,N,d,kind", [(256, 403, 512, "groups"), (96, 1100, 1024, "groups")])
def test_two_runs_are_bitwise_equal(dev, R, N, d, kind):
    q, k, qg, kg = contrastive_inputs(R, N, d, kind)
    assert _same(_run(dev, q, k, qg, kg, MIXED, 1.0 / R), _run(dev, q, k, qg, kg, MIXED, 1.0 / R))


@pytest.mark.parametrize("R,N,d,kind", [(33, 65, 64, "groups"), (256, 256, 512, "paired")])
def test_accumulate_is_bitwise_old_plus_fresh(dev, R, N, d, kind):
    q, k, qg, kg = contrastive_inputs(R, N, d, kind)
    fresh = _run(dev, q, k, qg, kg, MIXED, 1.0 / R)
    g = torch.Generator().manual_seed(3)
    old_q, old_k, old_h = (torch.randn(*s, generator=g).to(dev) for s in ((R, d), (N, d), (2,)))
    acc = _run(dev, q, k, qg, kg, MIXED, 1.0 / R, dq=old_q.clone(), dk=old_k.clone(), dhead=old_h.clone())
    assert _same(acc[:3], fresh[:3])
    assert torch.equal(acc[3], old_q + fresh[3]) and torch.equal(acc[4], old_k + fresh[4]) and torch.equal(acc[5], old_h + fresh[5])
    # ... and a passed buffer is overwritten where its flag says so
    over = _run(dev, q, k, qg, kg, MIXED, 1.0 / R, dq=old_q.clone(), dk=old_k.clone(), dhead=old_h.clone(),
                accumulate=(False, True, False))
    assert torch.equal(over[3], fresh[3]) and torch.equal(over[4], acc[4]) and torch.equal(over[5], fresh[5])


def test_loss_scale_record_multiplies_the_three_gradients_only(dev):
    from clipfs import ops
    q, k, qg, kg = contrastive_inputs(33, 65, 64, "groups")
    plain = _run(dev, q, k, qg, kg, MIXED, 1.0 / 33)
    state = ops.new_scaler_state(4096.0, dev)
    keep = state.clone()
    scaled = _run(dev, q, k, qg, kg, MIXED, 1.0 / 33, scale_state=state)
    assert _same(scaled[:3], plain[:3])
    for i in (3, 4, 5):
        assert torch.equal(scaled[i], plain[i] * 4096.0) and plain[i].abs().max().item() > 0
    assert torch.equal(state, keep)


def test_an_absent_gradient_leaves_the_others_unchanged(dev):
    q, k, qg, kg = contrastive_inputs(37, 83, 192, "groups")
    run = lambda **kw: _run(dev, q, k, qg, kg, MIXED, 1.0 / 37, **kw)
    every = run()
    for drop in (("dq",), ("dk",), ("dhead",), ("dq", "dk"), ("dq", "dk", "dhead")):
        out = run(**{f"want_{name}": False for name in drop})
        assert _same(out[:3], every[:3]), drop
        for i, name in ((3, "dq"), (4, "dk"), (5, "dhead")):
            assert (out[i] is None) if name in drop else torch.equal(out[i], every[i]), (drop, name)


@pytest.mark.parametrize("R,N,d", [(37, 83, 192), (4081, 40, 600)])
def test_poisoned_outputs_come_out_bitwise_equal(dev, R, N, d):
    """Every output the wrapper allocates pre-filled with 0, NaN and 1e30: row_stats included, every element is written."""
    q, k, qg, kg = contrastive_inputs(R, N, d, "groups")
    runs = []
    for fill in poison.FILLS:
        with poison.poisoned(fill):
            loss, rows, correct, dq, dk, dhead = _run(dev, q, k, qg, kg, MIXED, 1.0 / R)
        runs.append(dict(loss=loss, rows=rows[:3], best=rows[3].view(torch.int32), correct=correct, dq=dq, dk=dk, dhead=dhead))
    poison.assert_same_runs(runs)


@pytest.mark.parametrize("R,N,d", [(37, 83, 192), (33, 300, 64), (1, 1, 64)])
def test_guard_rows_are_untouched(dev, R, N, d):
    from clipfs import _lib, ops
    q, k, qg, kg = contrastive_inputs(R, N, d, "groups" if R > 1 else "paired")
    q, k, qg, kg, head = q.to(dev), k.to(dev), qg.to(dev), kg.to(dev), MIXED.to(dev)
    mark = 7.25
    rows = torch.full((4 * R + 8,), mark, device=dev)
    dq = torch.full((R + 2, d), mark, device=dev)
    dk = torch.full((N + 2, d), mark, device=dev)
    lsum = torch.full((4,), mark, device=dev)
    dhead = torch.full((6,), mark, device=dev)
    cor = torch.full((4,), 77, device=dev, dtype=torch.int32)
    rc = _lib.load().clipfs_sigmoid_objective(q.data_ptr(), k.data_ptr(), qg.data_ptr(), kg.data_ptr(), head.data_ptr(), 1.0 / R,
                                              None, rows.data_ptr() + 16, lsum.data_ptr(), cor.data_ptr(), dq[1:].data_ptr(), 0,
                                              dk[1:].data_ptr(), 0, dhead.data_ptr() + 8, 0, R, N, d,
                                              torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.load().clipfs_last_error()
    assert (rows[:4] == mark).all() and (rows[4 + 4 * R:] == mark).all()
    assert (dq[0] == mark).all() and (dq[R + 1] == mark).all() and (dk[0] == mark).all() and (dk[N + 1] == mark).all()
    assert (lsum[1:] == mark).all() and (cor[1:] == 77).all() and (dhead[:2] == mark).all() and (dhead[4:] == mark).all()
    want = ops.sigmoid_objective(q, k, qg, kg, head, 1.0 / R)
    assert poison.same_bits(rows[4:4 + 4 * R].view(4, R), want[1])
    assert torch.equal(dq[1:R + 1], want[3]) and torch.equal(dk[1:N + 1], want[4]) and torch.equal(dhead[2:4], want[5])
    assert lsum[0].item() == want[0].item() and cor[0].item() == want[2].item()


# ------------------------------------------------------------------------------------------- 4. the autograd Function
@pytest.mark.parametrize("B,M,d,kind", [(32, 32, 64, "paired"), (33, 65, 64, "groups"), (300, 40, 128, "groups")])
def test_siglip_loss_gradients(dev, B, M, d, kind):
    from clipfs import ops
    q, k, qg, kg = contrastive_inputs(B, M, d, kind)
    img, txt, head = q.to(dev).requires_grad_(), k.to(dev).requires_grad_(), MIXED.to(dev).requires_grad_()
    groups = (None, None) if kind == "paired" else (qg.to(dev), kg.to(dev))
    loss = ops.siglip_loss(img, txt, *groups, head=head)
    (3.0 * loss).backward()
    ref = sigmoid_ref(q, k, qg, kg, MIXED, 1.0 / B, scale=3.0)
    got = dict(loss=loss, rows=ref["rows"], dq=img.grad, dk=txt.grad, dhead=head.grad)  # the rows are not an output here
    err, bound = _errors(got, ref), _bounds("mixed")
    print(f"siglip_loss ({B}, {M}, {d}, {kind}): " + " ".join(f"{n} {err[n]:.2e}/{bound[n]:.2e}" for n in QUANTITIES))
    for name in ("loss", "dq", "dk", "dhead_t", "dhead_b"):
        assert err[name] <= bound[name], (name, err[name], bound[name])
    # an input that needs no gradient gets none, the others' are bitwise the same
    img2, head2 = q.to(dev).requires_grad_(), MIXED.to(dev).requires_grad_()
    (3.0 * ops.siglip_loss(img2, k.to(dev), *groups, head=head2)).backward()
    assert torch.equal(img2.grad, img.grad) and torch.equal(head2.grad, head.grad)


# ------------------------------------------------------------------------------------------- 5. the trainer against the oracle
HEADS = {"paired": (10.0, -10.0), "groups": (30.0, -8.0)}  # SigLIP's initial point; a point with cells off saturation


def _oracle_step(monkeypatch, cfg, sd, lw, img, cap, ig, cg, seed, p, t, b):
    """test_contrastive_gpu._oracle_step with the sigmoid loss in the place of the symmetric InfoNCE loss: (loss, adapter
    gradient blocks, fp64 gradient of (log t, b), the fp64 unit features)."""
    head = head_of(t, b).double().requires_grad_()
    monkeypatch.setattr(TC, "symmetric_loss", lambda feat, txt, g_i, g_c: sigmoid_loss(feat, txt, g_i, g_c, head, 1.0 / feat.shape[0]))
    want, blocks, feats = TC._oracle_step(cfg, sd, lw, img, cap, ig, cg, seed, p)
    return want, blocks, head.grad, feats


def _head_error(got, want, feats, ig, cg, t, b):
    """The head's two gradient entries against fp64 autograd, as shares of t sum |G a| and sum |G| of the fp64 features."""
    feat, txt = feats
    B, M = feat.shape[0], txt.shape[0]
    if ig is None:
        ig = cg = torch.arange(B, dtype=torch.int32)
    ref = sigmoid_ref(feat, txt, ig, cg, head_of(t, b), 1.0 / B)
    err = (got.detach().double().cpu() - want).abs()
    return float(err[0] / ref["scale_t"]), float(err[1] / ref["scale_b"]), ref


@pytest.mark.parametrize("kind,p", [("paired", 0.0), ("groups", 0.25)])
def test_step_pairs_against_oracle(dev, monkeypatch, kind, p):
    from clipfs.engine import _mix_seed
    L, cfg, sd, model, layers, lw = TC._model(dev, monkeypatch, p)
    img, cap, ig, cg = TC._batch(cfg, kind)
    t, b = HEADS[kind]
    model.train()
    tr = L.LoRAPairTrainer(model, pair_loss="sigmoid", pair_scale=t, pair_bias=b, train_pair_head=True)
    tr.flat.zero_grad()
    dg = lambda x: None if x is None else x.to(dev)
    loss, c_it, c_ti = tr.forward_backward_pairs(img.to(dev), cap.to(dev), dg(ig), dg(cg))
    seed = _mix_seed(model.engine.seed_base, model.engine.step)
    want, blocks, dhead, feats = _oracle_step(monkeypatch, cfg, sd, lw, img, cap, ig, cg, seed, p, t, b)
    e_loss = abs(loss.item() - want)
    e_grad = TC._grad_error(layers, blocks, types.SimpleNamespace(numel=tr.flat.numel - 2))  # the head: the last two
    e_t, e_b, ref = _head_error(tr.pair_head.grad_slot, dhead, feats, ig, cg, t, b)
    print(f"step_pairs sigmoid {kind} p={p}: loss {loss.item():.6f} err {e_loss:.3e} grad {e_grad:.3e} head {e_t:.3e} {e_b:.3e} "
          f"hits {c_it.item()} / {ref['correct']}")
    assert c_ti is None and tr.last_plan["vision"] is not None and tr.last_plan["text"] is not None
    assert tr.flat.segments[-1] == ("extra.0", 2) and tr.pair_head.grad_slot.data_ptr() == tr.flat.grads[-2:].data_ptr()
    assert e_loss <= TC.BOUND_TLOSS * max(1.0, abs(want)) and e_grad <= TC.BOUND_TGRAD
    assert e_t <= TC.BOUND_TGRAD and e_b <= TC.BOUND_TGRAD
    assert c_it.item() == ref["correct"]


def test_a_frozen_head_leaves_the_default_layout(dev, monkeypatch):
    layouts = {}
    for name, kw in (("default", {}), ("frozen", dict(pair_loss="sigmoid")), ("trained", dict(pair_loss="sigmoid", train_pair_head=True))):
        L, cfg, sd, model, layers, lw = TC._model(dev, monkeypatch)
        tr = (L.LoRATrainer if name == "default" else L.LoRAPairTrainer)(model, **kw)
        layouts[name] = (tr.flat.segments, tr.flat.numel)
        assert (tr.pair_head is None) == (name == "default")
        if name == "frozen":
            img, cap, ig, cg = (x.to(dev) for x in TC._batch(cfg, "groups"))
            before = tr.pair_head.data.clone()
            tr.step_pairs(img, cap, ig, cg)
            assert torch.equal(tr.pair_head.data, before) and not hasattr(tr.pair_head, "grad_slot")
            assert abs(tr.pair_scale_value - 10.0) < 1e-5 and tr.pair_bias_value == -10.0
    assert layouts["frozen"] == layouts["default"]
    plain = L.LoRAPairTrainer(TC._model(dev, monkeypatch)[3])  # pair_loss="infonce": a LoRATrainer in all but name
    assert (plain.flat.segments, plain.flat.numel) == layouts["default"] and plain.pair_loss == "infonce" and plain.pair_head is None
    assert layouts["trained"] == (layouts["default"][0] + [("extra.0", 2)], layouts["default"][1] + 2)
    with pytest.raises(ValueError, match="pair_loss must be"):
        L.LoRAPairTrainer(model, pair_loss="hinge")
    with pytest.raises(ValueError, match="train_pair_head needs"):
        L.LoRAPairTrainer(model, train_pair_head=True)
    with pytest.raises(ValueError, match="pair_scale must be positive"):
        L.LoRAPairTrainer(model, pair_loss="sigmoid", pair_scale=0.0)


def test_a_trained_head_moves_by_the_adamw_update_of_its_gradients(dev, monkeypatch):
    """First AdamW step: m-hat = g and v-hat = g^2, so p' = p - lr (g / (|g| + eps) + wd p).  The bound is four units in the
    last place of the larger entry, |b| = 10 (an fp32 step of a few roundings on a value of that size)."""
    L, cfg, sd, model, layers, lw = TC._model(dev, monkeypatch)
    img, cap, ig, cg = (x.to(dev) for x in TC._batch(cfg, "groups"))
    lr, wd, eps = 1e-2, 1e-2, 1e-8
    tr = L.LoRAPairTrainer(model, lr=lr, weight_decay=wd, eps=eps, pair_loss="sigmoid", pair_scale=30.0, pair_bias=-8.0,
                       train_pair_head=True)
    tr.flat.zero_grad()
    tr.forward_backward_pairs(img, cap, ig, cg)
    g, p0 = tr.pair_head.grad_slot.double().cpu(), tr.pair_head.data.double().cpu()
    tr.optimizer_step()
    want = p0 - lr * (g / (g.abs() + eps) + wd * p0)
    got = tr.pair_head.data.double().cpu()
    print("head", p0.tolist(), "grad", g.tolist(), "->", got.tolist(), "want", want.tolist())
    assert bool((g != 0).all()) and float((got - want).abs().max()) <= 4 * 2.0 ** -20
    assert float((got - p0).abs().min()) > 0.5 * lr
    assert abs(tr.pair_scale_value - math.exp(float(got[0]))) <= 1e-5 * tr.pair_scale_value and tr.pair_bias_value == float(got[1])


def test_three_scaled_steps_end_bitwise_on_the_unscaled_parameters(dev, monkeypatch):
    out = []
    for scale in (None, 2.0 ** 12):
        L, cfg, sd, model, layers, lw = TC._model(dev, monkeypatch, 0.25)
        img, cap, ig, cg = TC._batch(cfg, "groups")
        model.train()
        tr = L.LoRAPairTrainer(model, lr=1e-3, loss_scale=scale, pair_loss="sigmoid", pair_scale=30.0, pair_bias=-8.0,
                           train_pair_head=True)
        losses = [tr.step_pairs(img.to(dev), cap.to(dev), ig.to(dev), cg.to(dev))[0].item() for _ in range(3)]
        out.append((losses, tr.flat.params.clone()))
        assert tr.skipped_steps == 0 and tr.optimizer_steps == 3
    assert out[0][0] == out[1][0] and out[0][0][2] != out[0][0][0]
    assert torch.equal(out[0][1], out[1][1])
    assert not torch.equal(out[0][1][-2:].cpu(), head_of(30.0, -8.0))  # the head moved


def test_state_dict_round_trips_and_refuses_the_other_pair_loss(dev, monkeypatch):
    fresh = lambda: TC._model(dev, monkeypatch)  # a model of its own for every trainer
    L, cfg = fresh()[:2]
    img, cap, ig, cg = (x.to(dev) for x in TC._batch(cfg, "groups"))
    saved = {}
    for trained in (True, False):
        a = L.LoRAPairTrainer(fresh()[3], lr=1e-3, pair_loss="sigmoid", pair_scale=30.0, pair_bias=-8.0, train_pair_head=trained)
        a.step_pairs(img, cap, ig, cg)
        sd = saved[trained] = a.state_dict()
        assert sd["pair_loss"] == "sigmoid" and torch.equal(sd["pair_head"], a.pair_head.data.cpu())
        assert (("extra.0", 2) in sd["layout"]) == trained
        a.step_pairs(img, cap, ig, cg)
        b = L.LoRAPairTrainer(fresh()[3], pair_loss="sigmoid", pair_scale=2.0, pair_bias=0.0, train_pair_head=trained)
        b.load_state_dict(sd)
        assert torch.equal(b.pair_head.data.cpu(), sd["pair_head"])
        b.step_pairs(img, cap, ig, cg)
        assert torch.equal(b.flat.params, a.flat.params) and torch.equal(b.pair_head.data, a.pair_head.data)
    other = L.LoRATrainer(fresh()[3])
    assert other.state_dict()["pair_loss"] == "infonce" and other.state_dict()["pair_head"] is None
    with pytest.raises(ValueError, match="with pair_loss='sigmoid'"):
        other.load_state_dict(saved[False])
    with pytest.raises(ValueError, match="with pair_loss='infonce'"):
        b.load_state_dict(other.state_dict())
    c = L.LoRAPairTrainer(fresh()[3], pair_loss="sigmoid", train_pair_head=True)
    with pytest.raises(ValueError, match="extra.0: only in this trainer"):  # a trained head changes the layout fingerprint
        c.load_state_dict(saved[False])


# ------------------------------------------------------------------------------------------- 6. two ranks
def _dp_step(dev, monkey, kind, rank=0, world=1):
    from clipfs import dist as D
    L, cfg, sd, model, layers, lw = TC._model(dev, monkey)
    B, M = (TC.DP_B, TC.DP_M) if kind == "groups" else (TC.DP_B, TC.DP_B)
    img, cap, ig, cg = TC._batch(cfg, kind, B, M)
    model.eval()
    tr = L.LoRAPairTrainer(model, pair_loss="sigmoid", pair_scale=30.0, pair_bias=-8.0, train_pair_head=True)
    b0, b1 = D.block_bounds(B, rank, world)
    c0, c1 = D.block_bounds(M, rank, world)
    tr.flat.zero_grad()
    groups = (None, None) if ig is None else (ig[b0:b1].to(dev), cg[c0:c1].to(dev))
    out = tr.forward_backward_pairs(img[b0:b1].to(dev), cap[c0:c1].to(dev), *groups, B, M, row_offset=b0, caption_offset=c0)
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
    for kind, collectives in (("paired", 3), ("groups", 4)):
        tr, (loss, c_it, c_ti) = _dp_step(dev, TC._Monkey, kind, rank, world)
        assert (tr.rank, tr.world) == (rank, world) and c_ti is None
        assert tr.collectives_per_step == collectives, (kind, tr.collectives_per_step)
        tr.optimizer_step()  # the flat all-reduce: the ranks' shares of the head's gradient are summed with the rest
        total = torch.cat([loss, c_it.float()])
        D.allreduce_sum_(total)
        torch.cuda.synchronize()
        if rank == 0:
            np.savez(os.path.join(out_dir, f"sigmoid_{kind}.npz"), grads=tr.flat.grads.cpu().numpy(), total=total.cpu().numpy())
    dist.destroy_process_group()


def test_two_ranks_match_one_process(dev, monkeypatch, tmp_path):
    """7 images on two ranks against 7 captions (pairs) and 5 captions (groups): a padding row in the gathered caption
    table either way.  3 collectives for plain pairs, 4 with groups (asserted on the ranks)."""
    want = {}
    for kind in ("paired", "groups"):
        tr, (loss, c_it, _) = _dp_step(dev, monkeypatch, kind)
        assert tr.collectives_per_step == 0
        want[kind] = (tr.flat.grads.cpu().numpy(), loss.item(), c_it.item())
    mp.spawn(_pairs_rank, args=(2, TC._free_port(), str(tmp_path)), nprocs=2, join=True)
    for kind, (want_g, loss, hits) in want.items():
        z = np.load(os.path.join(str(tmp_path), f"sigmoid_{kind}.npz"))
        scale, hscale = np.abs(want_g[:-2]).max(), np.abs(want_g[-2:])
        e_loss = abs(float(z["total"][0]) - loss)
        e_grad = np.abs(z["grads"][:-2] - want_g[:-2]).max() / scale
        e_head = (np.abs(z["grads"][-2:] - want_g[-2:]) / hscale).max()
        print(f"two ranks sigmoid {kind}: loss {loss:.6f} err {e_loss:.3e} grad {e_grad:.3e} head {e_head:.3e} "
              f"hits {z['total'][1]} / {hits}")
        assert scale > 1e-5 and hscale.min() > 0
        assert e_loss <= TC.BOUND_DP_LOSS * max(1.0, abs(loss)) and e_grad <= TC.BOUND_DP_GRAD and e_head <= TC.BOUND_DP_GRAD
        assert int(z["total"][1]) == hits


# ------------------------------------------------------------------------------------------- 7. no host synchronisation
def test_step_pairs_does_not_synchronise(dev, monkeypatch):
    L, cfg, sd, model, layers, lw = TC._model(dev, monkeypatch, 0.25)
    img, cap, ig, cg = (t.to(dev) for t in TC._batch(cfg, "groups"))
    model.train()
    tr = L.LoRAPairTrainer(model, loss_scale=2.0 ** 12, max_grad_norm=1.0, pair_loss="sigmoid", train_pair_head=True)
    tr.step_pairs(img, cap, ig, cg)  # warm-up: the text tower's row plan of this caption table, the workspaces
    tr.step_pairs(img[:4].contiguous(), cap, None, None)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, c_it, c_ti = tr.step_pairs(img, cap, ig, cg)
        tr.step_pairs(img[:4].contiguous(), cap, None, None)  # pairs: the group vectors are made on the device
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(loss).all() and 0 <= c_it.item() <= 6 and c_ti is None
