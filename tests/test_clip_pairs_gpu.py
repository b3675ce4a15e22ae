"""The symmetric CLIP pair objective on the MI355X: clipfs_clip_pairs_objective against the fp64 reference of
clip_pairs_ref.py at three logit scales, symmetric and one-directional, its equivalence with
clipfs_contrastive_objective, its edge cases and exactness properties (bitwise run to run, accumulate = old + fresh, a
power-of-two loss scale, optional outputs, poisoned outputs, guard rows), ops.clip_pairs_loss, and LoRATrainer.step_pairs
under LoRAPairTrainer(pair_loss="clip") against fp64 autograd on the oracle, on two data-parallel ranks and without host
synchronisation.  The test model, the batches and the oracle step are those of test_contrastive_gpu.py.

Kernel bounds are not constants (the rule of test_sigmoid_gpu.py): per quantity and per s, 16 x the
worst error of the fp32 yardstick (the reference's own expressions evaluated in torch fp32 on the CPU) over the case
table, and at least 1e-6.  The yardstick is computed at run time, never from the kernels' output.  Error denominators:
max(1, |ref|) for loss_sum, lse and the row losses; the reference for 1 / n; the reference's largest entry for dq / dk;
sum |G z| for dhead, and the row's own sum_j |G z| for row 3 of the statistics.  Every test prints its figures before it
asserts.

Arg-max rule: a direction's hit count and best indices equal fp64 exactly where that direction's smallest top-1 / top-2
gap is at least 1e-5 s; elsewhere they may differ only on rows whose own fp64 gap is below 1e-5 s (at most 1 % of the rows;
test_clip_pairs_cpu.py asserts that of the case table).

Equivalence with clipfs_contrastive_objective at head = 0 (s = 1 exactly): loss_sum and correct are asserted EQUAL where
the older entry point's statistics are one key chunk (N <= 128: then both walk the keys in the same order and every
operation is the same), and the gradients bitwise; for N > 128 the older kernel merges per-chunk partials, which the new
one (no chunks: their partials would be scratch) cannot reproduce bit for bit, and the loss is held to the kernel rule.

Trainer bounds are the InfoNCE trainer's (test_contrastive_gpu.py: BOUND_TLOSS times max(1, loss), BOUND_TGRAD,
BOUND_DP_GRAD); the head's gradient entry is measured against sum |G z| of the fp64 features by the kernel rule.
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
from clip_pairs_ref import CASES, GAP, ONE_DIRECTIONAL, PEAKED, SCALES, clip_pairs_case, clip_pairs_ref, head_of
from contrastive_ref import contrastive_inputs, contrastive_loss

pytestmark = pytest.mark.gpu

FACTOR, FLOOR = 16.0, 1e-6
QUANTITIES = ("loss", "lse", "invn", "rows", "dz", "dq", "dk", "dhead")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _run(dev, q, k, qg, kg, head, wq, wk=0.0, **kw):
    from clipfs import ops
    for name in ("dq", "dk", "dhead", "scale_state"):
        if kw.get(name) is not None:
            kw[name] = kw[name].to(dev)
    return ops.clip_pairs_objective(q.to(dev), k.to(dev), qg.to(dev), kg.to(dev), head.to(dev), wq, wk, **kw)


def _as_dict(out):
    loss, qs, ks, correct, dq, dk, dhead = out
    best = lambda st: None if st is None else st[4].view(torch.int32).long().cpu()
    return dict(loss=loss[0], qstats=qs, kstats=ks, dq=dq, dk=dk, dhead=None if dhead is None else dhead[0],
                correct=tuple(correct.tolist()), qbest=best(qs), kbest=best(ks))


def _yard_as_got(yard):
    side = lambda s: None if s is None else s["rows"]
    return dict(loss=yard["loss"], qstats=side(yard["qside"]), kstats=side(yard["kside"]), dq=yard["dq"], dk=yard["dk"],
                dhead=yard["dhead"])


def _ratio(err, den):
    m = den > 0
    return float((err[m] / den[m]).max()) if bool(m.any()) else 0.0


def _errors(got, ref):
    """The error figures of ``got`` (kernel outputs or the fp32 yardstick) against the fp64 reference ``ref``; the
    statistics figures are the worse of the two sides."""
    f = lambda x: x.detach().double().cpu()
    top = lambda x: float(x.abs().max())
    one = lambda x: x.abs().clamp(min=1.0)
    err = dict.fromkeys(QUANTITIES, 0.0)
    err["loss"] = float((f(got["loss"]) - ref["loss"]).abs() / max(1.0, abs(float(ref["loss"]))))
    for stats, side in ((got["qstats"], ref["qside"]), (got["kstats"], ref["kside"])):
        if side is None:
            continue
        rows, want, alive = f(stats), side["rows"], side["alive"]
        if bool(alive.any()):
            err["lse"] = max(err["lse"], float(((rows[0] - want[0]).abs() / one(want[0]))[alive].max()))
            err["invn"] = max(err["invn"], float(((rows[1] - want[1]).abs() / want[1])[alive].max()))
            err["rows"] = max(err["rows"], float(((rows[2] - want[2]).abs() / one(want[2]))[alive].max()))
        err["dz"] = max(err["dz"], _ratio((rows[3] - want[3]).abs(), side["dz_rows_scale"]))
    for name in ("dq", "dk"):
        if top(ref[name]) > 0:
            err[name] = top(f(got[name]) - ref[name]) / top(ref[name])
    if float(ref["dhead_scale"]) > 0:
        err["dhead"] = float((f(got["dhead"]) - ref["dhead"]).abs() / ref["dhead_scale"])
    return err


@functools.lru_cache(maxsize=None)
def _bounds(s):
    """{quantity: bound} at one s: FACTOR x the yardstick's worst error over the case table (the one peaked case at its own
    s), at least FLOOR."""
    cases = [(PEAKED[0], dict(honest=False))] if s == PEAKED[1] else [(c, {}) for c in CASES]
    worst = dict.fromkeys(QUANTITIES, 0.0)
    for case, kw in cases:
        *_, ref, yard = clip_pairs_case(*case, s, **kw)
        for name, e in _errors(_yard_as_got(yard), ref).items():
            worst[name] = max(worst[name], e)
    return {name: max(FACTOR * e, FLOOR) for name, e in worst.items()}


def _check_hits(got_best, got_correct, side, s, tag):
    """The arg-max rule of the module docstring for one direction."""
    want_best = side["best"]
    close = side["gaps"] < GAP * s
    differ = got_best != want_best
    print(f"{tag}: correct {got_correct} / {side['correct']}, best differs on {int(differ.sum())} rows, "
          f"{int(close.sum())} rows below the gap")
    if not bool(close.any()):
        assert not bool(differ.any()) and got_correct == side["correct"]
        return
    assert int(close.sum()) * 100 <= len(close)
    assert not bool((differ & ~close).any())
    assert abs(got_correct - side["correct"]) <= int((differ & close).sum())


def _check(got, ref, s, tag):
    err, bound = _errors(got, ref), _bounds(s)
    print(f"{tag} [s = {s:.4g}]: " + " ".join(f"{n} {err[n]:.2e}/{bound[n]:.2e}" for n in QUANTITIES))
    for stats, best, side, hits, name in ((got["qstats"], got["qbest"], ref["qside"], got["correct"][0], "q"),
                                          (got["kstats"], got["kbest"], ref["kside"], got["correct"][1], "k")):
        if side is None:
            assert stats is None and hits == 0
            continue
        dead = ~side["alive"]
        st = stats.cpu()
        assert bool((st[0][dead] == float("inf")).all()) and bool((st[1:4][:, dead] == 0).all()), "a row that contributes nothing"
        _check_hits(best, hits, side, s, f"{tag} {name} side")
    for name in QUANTITIES:
        assert err[name] <= bound[name], (tag, s, name, err[name], bound[name])
    return err


# ------------------------------------------------------------------------------------------- 1. kernel against the reference
@pytest.mark.parametrize("R,N,d,kind", CASES)
@pytest.mark.parametrize("name", list(SCALES))
def test_kernel_against_reference(dev, R, N, d, kind, name):
    s = SCALES[name]
    q, k, qg, kg, head, ref, _ = clip_pairs_case(R, N, d, kind, s)
    _check(_as_dict(_run(dev, q, k, qg, kg, head, 0.5 / R, 0.5 / N)), ref, s, f"({R}, {N}, {d}, {kind})")


@pytest.mark.parametrize("R,N,d,kind", ONE_DIRECTIONAL)
@pytest.mark.parametrize("name", list(SCALES))
def test_one_directional_kernel_against_reference(dev, R, N, d, kind, name):
    s = SCALES[name]
    q, k, qg, kg, head, ref, _ = clip_pairs_case(R, N, d, kind, s, both=False)
    got = _as_dict(_run(dev, q, k, qg, kg, head, 1.0 / R))
    assert got["kstats"] is None and got["correct"][1] == 0
    _check(got, ref, s, f"one direction ({R}, {N}, {d}, {kind})")


def test_peaked_case(dev):
    (R, N, d, kind), s = PEAKED
    q, k, qg, kg, head, ref, _ = clip_pairs_case(R, N, d, kind, s, honest=False)
    _check(_as_dict(_run(dev, q, k, qg, kg, head, 0.5 / R, 0.5 / N)), ref, s, f"peaked ({R}, {N}, {d}, {kind})")


def test_key_side_is_the_query_side_of_the_swapped_call(dev):
    """One z per cell in both roles: the key statistics of a symmetric call are bitwise the query statistics of the call
    with q and k exchanged, and its gradients are bitwise those of that call exchanged."""
    q, k, qg, kg = contrastive_inputs(256, 403, 512, "groups")
    head = head_of(100.0)
    a = _run(dev, q, k, qg, kg, head, 0.5 / 256, 0.5 / 403)
    b = _run(dev, k, q, kg, qg, head, 0.5 / 403, 0.5 / 256)
    assert poison.same_bits(a[1], b[2]) and poison.same_bits(a[2], b[1])
    assert a[3].tolist() == b[3].tolist()[::-1]
    same = torch.equal(a[4], b[5]) and torch.equal(a[5], b[4])
    print("swapped call: statistics bitwise equal; gradients bitwise equal:", same,
          float((a[4] - b[5]).abs().max()), float((a[5] - b[4]).abs().max()))
    assert same


# ------------------------------------------------------------------------------------------- 2. equivalence at s = 1
@pytest.mark.parametrize("R,N,d,kind", [(33, 65, 64, "groups"), (300, 40, 128, "groups"), (256, 403, 512, "groups")])
def test_one_directional_call_is_the_contrastive_objective_at_head_zero(dev, R, N, d, kind):
    from clipfs import ops
    q, k, qg, kg = (x.to(dev) for x in contrastive_inputs(R, N, d, kind))
    head = torch.zeros(1, device=dev)
    loss, qs, ks, correct, dq, dk, dhead = ops.clip_pairs_objective(q, k, qg, kg, head, 1.0 / R)
    l0, rows0, c0, dq0, dk0 = ops.contrastive_objective(q, k, qg, kg, 1.0, 1.0 / R, accumulate=False)
    chunks = ops.contrastive_plan("stats", R, N, d)["chunks"]
    bitwise = torch.equal(dq, dq0) and torch.equal(dk, dk0)
    print(f"({R}, {N}, {d}) chunks {chunks}: loss {loss.item()!r} / {l0.item()!r} correct {correct.tolist()} / {c0.item()} "
          f"rows equal {torch.equal(qs[2], rows0)} gradients bitwise {bitwise}")
    assert correct[0].item() == c0.item() and correct[1].item() == 0 and ks is None
    ref = clip_pairs_ref(q.cpu(), k.cpu(), qg.cpu(), kg.cpu(), head.cpu(), 1.0 / R)
    bound = _bounds(1.0)
    top = lambda x: float(x.abs().max())
    for got, want, name in ((dq, dq0, "dq"), (dk, dk0, "dk")):
        assert top(got.double().cpu() - want.double().cpu()) / top(ref[name]) <= bound[name], name
    if chunks == 1:
        assert loss.item() == l0.item() and torch.equal(qs[2], rows0) and bitwise
    else:
        assert abs(loss.item() - l0.item()) / max(1.0, abs(float(ref["loss"]))) <= bound["loss"]


# ------------------------------------------------------------------------------------------- 3. edge cases
HEAD = head_of(100.0)


def test_every_key_masked(dev):
    R, N, d = 37, 83, 192
    q, k, qg, _ = contrastive_inputs(R, N, d, "groups")
    kg = torch.full((N,), -1, dtype=torch.int32)
    old = torch.full((1,), 3.0)
    loss, qs, ks, correct, dq, dk, dhead = _run(dev, q, k, qg, kg, HEAD, 0.5 / R, 0.5 / N, dhead=old.clone(), accumulate=True)
    print("every key masked:", loss.item(), correct.tolist(), dq.abs().max().item(), dk.abs().max().item(), dhead.tolist())
    assert loss.item() == 0 and correct.tolist() == [0, 0]
    for st in (qs, ks):
        assert bool((st[0] == float("inf")).all()) and bool((st[1:4] == 0).all())
    assert bool((qs[4].view(torch.int32) == -1).all()) and bool((ks[4].view(torch.int32) == -1).all())
    assert dq.abs().max().item() == 0 and dk.abs().max().item() == 0 and torch.equal(dhead.cpu(), old)


def test_every_query_masked_but_one(dev):
    R, N, d = 33, 65, 64
    q, k, qg, kg = contrastive_inputs(R, N, d, "groups")
    keep = int((qg >= 0).nonzero()[5])
    g = int(qg[keep])
    qg = torch.full_like(qg, -1)
    qg[keep] = g
    kg[:4] = g
    ref = clip_pairs_ref(q, k, qg, kg, HEAD, 0.5 / R, 0.5 / N)
    got = _as_dict(_run(dev, q, k, qg, kg, HEAD, 0.5 / R, 0.5 / N))
    _check(got, ref, 100.0, "all queries masked but one")
    dead = torch.arange(R) != keep
    assert got["dq"].cpu()[dead].abs().max().item() == 0 and bool((got["qbest"][dead] == -1).all())
    assert got["dk"].cpu()[kg < 0].abs().max().item() == 0
    # a key's only live query is its best one; a key of another group has a loss of 0 (one live query: softmax 1)
    assert bool((got["kbest"][kg >= 0] == keep).all()) and got["correct"][1] == int((kg == g).sum())


def test_no_positive_anywhere(dev):
    R, N, d = 37, 83, 192
    q, k, _, _ = contrastive_inputs(R, N, d, "groups")
    qg, kg = torch.full((R,), 5, dtype=torch.int32), torch.full((N,), 7, dtype=torch.int32)
    kg[::9] = -1
    loss, qs, ks, correct, dq, dk, dhead = _run(dev, q, k, qg, kg, HEAD, 0.5 / R, 0.5 / N)
    print("no positive:", loss.item(), correct.tolist(), dq.abs().max().item(), dk.abs().max().item(), dhead.item())
    assert loss.item() == 0 and correct.tolist() == [0, 0] and dhead.item() == 0
    assert dq.abs().max().item() == 0 and dk.abs().max().item() == 0
    assert bool((qs[4].view(torch.int32) >= 0).all())  # live rows still have a best key


def test_identical_keys_give_index_zero(dev):
    R, N, d = 40, 70, 64
    q, k, _, _ = contrastive_inputs(R, N, d, "groups")
    k = k[3:4].repeat(N, 1).contiguous()
    qg, kg = (torch.arange(R) % 3).to(torch.int32), ((torch.arange(N) + 1) % 3).to(torch.int32)
    got = _as_dict(_run(dev, q, k, qg, kg, HEAD, 0.5 / R, 0.5 / N))
    print("identical keys: best", got["qbest"].unique().tolist(), "correct", got["correct"])
    assert bool((got["qbest"] == 0).all()) and got["correct"][0] == int((qg == kg[0]).sum())
    # every key sees the same column of logits: one best query for all of them
    assert len(got["kbest"].unique()) == 1


# ------------------------------------------------------------------------------------------- 4. exactness
def _same(a, b):
    return all((x is None and y is None) or poison.same_bits(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("R,N,d,kind", [(256, 403, 512, "groups"), (96, 1100, 1024, "groups")])
def test_two_runs_are_bitwise_equal(dev, R, N, d, kind):
    q, k, qg, kg = contrastive_inputs(R, N, d, kind)
    assert _same(_run(dev, q, k, qg, kg, HEAD, 0.5 / R, 0.5 / N), _run(dev, q, k, qg, kg, HEAD, 0.5 / R, 0.5 / N))


@pytest.mark.parametrize("R,N,d,kind", [(33, 65, 64, "groups"), (256, 256, 512, "paired")])
def test_accumulate_is_bitwise_old_plus_fresh(dev, R, N, d, kind):
    q, k, qg, kg = contrastive_inputs(R, N, d, kind)
    fresh = _run(dev, q, k, qg, kg, HEAD, 0.5 / R, 0.5 / N)
    g = torch.Generator().manual_seed(3)
    old_q, old_k, old_h = (torch.randn(*s, generator=g).to(dev) for s in ((R, d), (N, d), (1,)))
    acc = _run(dev, q, k, qg, kg, HEAD, 0.5 / R, 0.5 / N, dq=old_q.clone(), dk=old_k.clone(), dhead=old_h.clone(), accumulate=True)
    assert _same(acc[:4], fresh[:4])
    assert torch.equal(acc[4], old_q + fresh[4]) and torch.equal(acc[5], old_k + fresh[5]) and torch.equal(acc[6], old_h + fresh[6])
    # ... a passed buffer is overwritten by default, and where its flag says so
    over = _run(dev, q, k, qg, kg, HEAD, 0.5 / R, 0.5 / N, dq=old_q.clone(), dk=old_k.clone(), dhead=old_h.clone(),
                accumulate=(False, True, False))
    assert torch.equal(over[4], fresh[4]) and torch.equal(over[5], acc[5]) and torch.equal(over[6], fresh[6])
    plain = _run(dev, q, k, qg, kg, HEAD, 0.5 / R, 0.5 / N, dq=old_q.clone(), dk=old_k.clone(), dhead=old_h.clone())
    assert _same(plain, fresh)


def test_loss_scale_record_multiplies_the_three_gradients_only(dev):
    from clipfs import ops
    q, k, qg, kg = contrastive_inputs(33, 65, 64, "groups")
    plain = _run(dev, q, k, qg, kg, HEAD, 0.5 / 33, 0.5 / 65)
    state = ops.new_scaler_state(4096.0, dev)
    keep = state.clone()
    scaled = _run(dev, q, k, qg, kg, HEAD, 0.5 / 33, 0.5 / 65, scale_state=state)
    assert _same(scaled[:4], plain[:4])
    for i in (4, 5, 6):
        assert torch.equal(scaled[i], plain[i] * 4096.0) and plain[i].abs().max().item() > 0
    assert torch.equal(state, keep)


def test_an_absent_gradient_leaves_the_others_unchanged(dev):
    q, k, qg, kg = contrastive_inputs(37, 83, 192, "groups")
    run = lambda **kw: _run(dev, q, k, qg, kg, HEAD, 0.5 / 37, 0.5 / 83, **kw)
    every = run()
    for drop in (("dq",), ("dk",), ("dhead",), ("dq", "dk"), ("dq", "dk", "dhead")):
        out = run(**{f"want_{name}": False for name in drop})
        assert _same(out[:4], every[:4]), drop
        for i, name in ((4, "dq"), (5, "dk"), (6, "dhead")):
            assert (out[i] is None) if name in drop else torch.equal(out[i], every[i]), (drop, name)


@pytest.mark.parametrize("R,N,d", [(37, 83, 192), (4081, 40, 600)])
def test_poisoned_outputs_come_out_bitwise_equal(dev, R, N, d):
    """Every output the wrapper allocates pre-filled with 0, NaN and 1e30: both statistics arrays included, every element
    is written.  (lse is +inf on rows that contribute nothing: it is compared by bits with the indices, not as a finite
    float.)"""
    q, k, qg, kg = contrastive_inputs(R, N, d, "groups")
    runs = []
    for fill in poison.FILLS:
        with poison.poisoned(fill):
            loss, qs, ks, correct, dq, dk, dhead = _run(dev, q, k, qg, kg, HEAD, 0.5 / R, 0.5 / N)
        runs.append(dict(loss=loss, qrows=qs[1:4], krows=ks[1:4], qbits=qs[[0, 4]].view(torch.int32),
                         kbits=ks[[0, 4]].view(torch.int32), correct=correct, dq=dq, dk=dk, dhead=dhead))
    poison.assert_same_runs(runs)


@pytest.mark.parametrize("R,N,d", [(37, 83, 192), (33, 300, 64), (1, 1, 64)])
def test_guard_rows_are_untouched(dev, R, N, d):
    from clipfs import _lib, ops
    q, k, qg, kg = contrastive_inputs(R, N, d, "groups" if R > 1 else "paired")
    q, k, qg, kg, head = q.to(dev), k.to(dev), qg.to(dev), kg.to(dev), HEAD.to(dev)
    mark = 7.25
    qs = torch.full((5 * R + 8,), mark, device=dev)
    ks = torch.full((5 * N + 8,), mark, device=dev)
    dq = torch.full((R + 2, d), mark, device=dev)
    dk = torch.full((N + 2, d), mark, device=dev)
    lsum = torch.full((4,), mark, device=dev)
    dhead = torch.full((5,), mark, device=dev)
    cor = torch.full((5,), 77, device=dev, dtype=torch.int32)
    rc = _lib.load().clipfs_clip_pairs_objective(q.data_ptr(), k.data_ptr(), qg.data_ptr(), kg.data_ptr(), head.data_ptr(),
                                                 0.5 / R, 0.5 / N, None, qs.data_ptr() + 16, ks.data_ptr() + 16, lsum.data_ptr(),
                                                 cor.data_ptr(), dq[1:].data_ptr(), 0, dk[1:].data_ptr(), 0, dhead.data_ptr() + 8,
                                                 0, R, N, d, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.load().clipfs_last_error()
    assert (qs[:4] == mark).all() and (qs[4 + 5 * R:] == mark).all() and (ks[:4] == mark).all() and (ks[4 + 5 * N:] == mark).all()
    assert (dq[0] == mark).all() and (dq[R + 1] == mark).all() and (dk[0] == mark).all() and (dk[N + 1] == mark).all()
    assert (lsum[1:] == mark).all() and (cor[2:] == 77).all() and (dhead[:2] == mark).all() and (dhead[3:] == mark).all()
    want = ops.clip_pairs_objective(q, k, qg, kg, head, 0.5 / R, 0.5 / N)
    assert poison.same_bits(qs[4:4 + 5 * R].view(5, R), want[1]) and poison.same_bits(ks[4:4 + 5 * N].view(5, N), want[2])
    assert torch.equal(dq[1:R + 1], want[4]) and torch.equal(dk[1:N + 1], want[5]) and torch.equal(dhead[2:3], want[6])
    assert lsum[0].item() == want[0].item() and cor[:2].tolist() == want[3].tolist()


# ------------------------------------------------------------------------------------------- 5. the autograd Function
@pytest.mark.parametrize("B,M,d,kind", [(32, 32, 64, "paired"), (33, 65, 64, "groups"), (300, 40, 128, "groups")])
def test_clip_pairs_loss_gradients(dev, B, M, d, kind):
    from clipfs import ops
    q, k, qg, kg = contrastive_inputs(B, M, d, kind)
    img, txt, head = q.to(dev).requires_grad_(), k.to(dev).requires_grad_(), HEAD.to(dev).requires_grad_()
    groups = (None, None) if kind == "paired" else (qg.to(dev), kg.to(dev))
    loss = ops.clip_pairs_loss(img, txt, *groups, head=head)
    (3.0 * loss).backward()
    ref = clip_pairs_ref(q, k, qg, kg, HEAD, 0.5 / B, 0.5 / M, scale=3.0)
    got = dict(loss=loss, qstats=ref["qside"]["rows"], kstats=ref["kside"]["rows"], dq=img.grad, dk=txt.grad, dhead=head.grad[0])
    err, bound = _errors(got, ref), _bounds(100.0)
    print(f"clip_pairs_loss ({B}, {M}, {d}, {kind}): " + " ".join(f"{n} {err[n]:.2e}/{bound[n]:.2e}" for n in QUANTITIES))
    for name in ("loss", "dq", "dk", "dhead"):
        assert err[name] <= bound[name], (name, err[name], bound[name])
    # an input that needs no gradient gets none, the others' are bitwise the same
    img2, head2 = q.to(dev).requires_grad_(), HEAD.to(dev).requires_grad_()
    (3.0 * ops.clip_pairs_loss(img2, k.to(dev), *groups, head=head2)).backward()
    assert torch.equal(img2.grad, img.grad) and torch.equal(head2.grad, head.grad)


# ------------------------------------------------------------------------------------------- 6. the trainer against the oracle
def _clip_loss(feat, txt, g_i, g_c, head):
    s = torch.exp(head[0])
    return (contrastive_loss(feat, txt, g_i, g_c, s, 0.5 / feat.shape[0]) + contrastive_loss(txt, feat, g_c, g_i, s, 0.5 / txt.shape[0]))


def _oracle_step(monkeypatch, cfg, sd, lw, img, cap, ig, cg, seed, p, s):
    """test_contrastive_gpu._oracle_step at the scale exp(head[0]) of a leaf ``head``: (loss, adapter gradient blocks, fp64
    gradient of log s, the fp64 unit features)."""
    head = head_of(s).double().requires_grad_()
    monkeypatch.setattr(TC, "symmetric_loss", lambda feat, txt, g_i, g_c: _clip_loss(feat, txt, g_i, g_c, head))
    want, blocks, feats = TC._oracle_step(cfg, sd, lw, img, cap, ig, cg, seed, p)
    return want, blocks, head.grad, feats


def _head_ref(feats, ig, cg, s):
    feat, txt = feats
    B, M = feat.shape[0], txt.shape[0]
    if ig is None:
        ig = cg = torch.arange(B, dtype=torch.int32)
    return clip_pairs_ref(feat, txt, ig, cg, head_of(s), 0.5 / B, 0.5 / M)


@pytest.mark.parametrize("kind,p", [("paired", 0.0), ("groups", 0.25)])
def test_step_pairs_against_oracle(dev, monkeypatch, kind, p):
    from clipfs.engine import _mix_seed
    L, cfg, sd, model, layers, lw = TC._model(dev, monkeypatch, p)
    img, cap, ig, cg = TC._batch(cfg, kind)
    s = 100.0
    model.train()
    tr = L.LoRAPairTrainer(model, logit_scale=s, pair_loss="clip", train_pair_head=True)
    tr.flat.zero_grad()
    dg = lambda x: None if x is None else x.to(dev)
    loss, c_it, c_ti = tr.forward_backward_pairs(img.to(dev), cap.to(dev), dg(ig), dg(cg))
    seed = _mix_seed(model.engine.seed_base, model.engine.step)
    want, blocks, dhead, feats = _oracle_step(monkeypatch, cfg, sd, lw, img, cap, ig, cg, seed, p, s)
    ref = _head_ref(feats, ig, cg, s)
    e_loss = abs(loss.item() - want)
    e_grad = TC._grad_error(layers, blocks, types.SimpleNamespace(numel=tr.flat.numel - 1))  # the head: the last entry
    e_head = abs(tr.pair_head.grad_slot.double().cpu().item() - dhead.item()) / float(ref["dhead_scale"])
    bound = _bounds(s)["dhead"]
    print(f"step_pairs clip {kind} p={p}: loss {loss.item():.6f} err {e_loss:.3e} grad {e_grad:.3e} head {e_head:.3e}/{bound:.3e} "
          f"(dhead {dhead.item():.4e}, sum |G z| {float(ref['dhead_scale']):.4e}) hits {c_it.item()} {c_ti.item()} / {ref['correct']}")
    assert tr.last_plan["vision"] is not None and tr.last_plan["text"] is not None
    assert tr.flat.segments[-1] == ("extra.0", 1) and tr.pair_head.grad_slot.data_ptr() == tr.flat.grads[-1:].data_ptr()
    assert e_loss <= TC.BOUND_TLOSS * max(1.0, abs(want)) and e_grad <= TC.BOUND_TGRAD
    assert e_head <= bound
    assert (c_it.item(), c_ti.item()) == ref["correct"]


def test_a_frozen_head_leaves_the_default_layout(dev, monkeypatch):
    layouts = {}
    for name, kw in (("default", {}), ("frozen", dict(pair_loss="clip")), ("trained", dict(pair_loss="clip", train_pair_head=True))):
        L, cfg, sd, model, layers, lw = TC._model(dev, monkeypatch)
        tr = (L.LoRATrainer if name == "default" else L.LoRAPairTrainer)(model, **kw)
        layouts[name] = (tr.flat.segments, tr.flat.numel)
        assert (tr.pair_head is None) == (name == "default")
        assert (tr.tail_update is not None) == (name == "trained")
        if name == "frozen":
            img, cap, ig, cg = (x.to(dev) for x in TC._batch(cfg, "groups"))
            before = tr.pair_head.data.clone()
            tr.step_pairs(img, cap, ig, cg)
            assert torch.equal(tr.pair_head.data, before) and not hasattr(tr.pair_head, "grad_slot")
            assert abs(tr.pair_scale_value - 100.0) < 1e-3 and tr.pair_bias_value is None
    assert layouts["frozen"] == layouts["default"]
    assert layouts["trained"] == (layouts["default"][0] + [("extra.0", 1)], layouts["default"][1] + 1)
    with pytest.raises(ValueError, match="train_pair_head needs"):
        L.LoRAPairTrainer(model, train_pair_head=True)
    with pytest.raises(ValueError, match="pair_scale belongs"):
        L.LoRAPairTrainer(model, pair_loss="clip", pair_scale=30.0)
    with pytest.raises(ValueError, match="pair_bias belongs"):
        L.LoRAPairTrainer(model, pair_loss="clip", pair_bias=-8.0)
    with pytest.raises(ValueError, match="pair_scale_max needs"):
        L.LoRAPairTrainer(model, pair_loss="sigmoid", pair_scale_max=50.0)
    # the sigmoid head keeps the plain launch unless it is given a decay of its own
    assert L.LoRAPairTrainer(TC._model(dev, monkeypatch)[3], pair_loss="sigmoid", train_pair_head=True).tail_update is None
    own = L.LoRAPairTrainer(TC._model(dev, monkeypatch)[3], pair_loss="sigmoid", train_pair_head=True, pair_head_weight_decay=0.0)
    assert own.tail_update == (2, 0.0, -math.inf, math.inf)


def test_a_trained_head_moves_by_the_adamw_update_with_decay_zero(dev, monkeypatch):
    """First AdamW step: m-hat = g and v-hat = g^2, so p' = p - lr g / (|g| + eps), and no decay term on the head.  The
    bound is four units in the last place of log 30 (an fp32 step of a few roundings on a value of that size)."""
    L, cfg, sd, model, layers, lw = TC._model(dev, monkeypatch)
    img, cap, ig, cg = (x.to(dev) for x in TC._batch(cfg, "groups"))
    lr, wd, eps = 1e-2, 0.5, 1e-8  # a decay that would show: lr wd log 30 = 1.7e-2
    tr = L.LoRAPairTrainer(model, lr=lr, weight_decay=wd, eps=eps, logit_scale=30.0, pair_loss="clip", train_pair_head=True)
    assert tr.tail_update == (1, 0.0, -math.inf, math.log(100.0))
    tr.flat.zero_grad()
    tr.forward_backward_pairs(img, cap, ig, cg)
    g, p0 = tr.pair_head.grad_slot.double().cpu(), tr.pair_head.data.double().cpu()
    body0, gbody = tr.flat.params[:-1].double().cpu(), tr.flat.grads[:-1].double().cpu()
    tr.optimizer_step()
    want = p0 - lr * g / (g.abs() + eps)
    got = tr.pair_head.data.double().cpu()
    print("head", p0.tolist(), "grad", g.tolist(), "->", got.tolist(), "want", want.tolist())
    assert g.item() != 0 and float((got - want).abs().max()) <= 4 * 2.0 ** -22
    assert abs(tr.pair_scale_value - math.exp(float(got[0]))) <= 1e-5 * tr.pair_scale_value
    # ... while the body is decayed as before
    moved = gbody != 0
    want_body = body0 - lr * (gbody / (gbody.abs() + eps) + wd * body0)
    assert float((tr.flat.params[:-1].double().cpu() - want_body)[moved].abs().max()) <= 1e-6


def test_the_clamp_holds_log_s_at_its_cap(dev, monkeypatch):
    """logit_scale = pair_scale_max = 100: a step that would raise log s leaves it at log 100, one that lowers it moves."""
    L, cfg, sd, model, layers, lw = TC._model(dev, monkeypatch)
    img, cap, ig, cg = (x.to(dev) for x in TC._batch(cfg, "groups"))
    tr = L.LoRAPairTrainer(model, lr=1e-2, logit_scale=100.0, pair_loss="clip", train_pair_head=True, pair_scale_max=100.0)
    cap_value = torch.tensor([math.log(100.0)], dtype=torch.float32)
    start = tr.pair_head.data.cpu().clone()
    tr.flat.zero_grad()
    tr.forward_backward_pairs(img, cap, ig, cg)
    tr.pair_head.grad_slot.copy_(-tr.pair_head.grad_slot.abs() - 1.0)  # a gradient that raises log s, whatever the batch says
    tr.optimizer_step()
    after = tr.pair_head.data.cpu().clone()
    print("clamp: start", start.item(), "after a raising step", after.item(), "cap", cap_value.item())
    assert after.item() <= cap_value.item() and abs(after.item() - cap_value.item()) <= 2.0 ** -21
    free = L.LoRAPairTrainer(TC._model(dev, monkeypatch)[3], lr=1e-2, logit_scale=100.0, pair_loss="clip", train_pair_head=True,
                             pair_scale_max=None)
    free.flat.zero_grad()
    free.forward_backward_pairs(img, cap, ig, cg)
    free.pair_head.grad_slot.copy_(-free.pair_head.grad_slot.abs() - 1.0)
    free.optimizer_step()
    assert free.pair_head.data.item() > cap_value.item() + 5e-3
    assert free.tail_update == (1, 0.0, -math.inf, math.inf)  # no clamp, but still its own decay (the buffer's is 1e-2)


def test_three_scaled_steps_end_bitwise_on_the_unscaled_parameters(dev, monkeypatch):
    out = []
    for scale in (None, 2.0 ** 12):
        L, cfg, sd, model, layers, lw = TC._model(dev, monkeypatch, 0.25)
        img, cap, ig, cg = TC._batch(cfg, "groups")
        model.train()
        tr = L.LoRAPairTrainer(model, lr=1e-3, loss_scale=scale, logit_scale=30.0, pair_loss="clip", train_pair_head=True)
        losses = [tr.step_pairs(img.to(dev), cap.to(dev), ig.to(dev), cg.to(dev))[0].item() for _ in range(3)]
        out.append((losses, tr.flat.params.clone()))
        assert tr.skipped_steps == 0 and tr.optimizer_steps == 3
    assert out[0][0] == out[1][0] and out[0][0][2] != out[0][0][0]
    assert torch.equal(out[0][1], out[1][1])
    assert not torch.equal(out[0][1][-1:].cpu(), head_of(30.0))  # the head moved


def test_state_dict_round_trips_and_refuses_the_other_pair_losses(dev, monkeypatch):
    fresh = lambda: TC._model(dev, monkeypatch)  # a model of its own for every trainer
    L, cfg = fresh()[:2]
    img, cap, ig, cg = (x.to(dev) for x in TC._batch(cfg, "groups"))
    saved = {}
    for trained in (True, False):
        a = L.LoRAPairTrainer(fresh()[3], lr=1e-3, logit_scale=30.0, pair_loss="clip", train_pair_head=trained)
        a.step_pairs(img, cap, ig, cg)
        sd = saved[trained] = a.state_dict()
        assert sd["pair_loss"] == "clip" and torch.equal(sd["pair_head"], a.pair_head.data.cpu())
        assert (("extra.0", 1) in sd["layout"]) == trained
        a.step_pairs(img, cap, ig, cg)
        b = L.LoRAPairTrainer(fresh()[3], logit_scale=2.0, pair_loss="clip", train_pair_head=trained)
        b.load_state_dict(sd)
        assert torch.equal(b.pair_head.data.cpu(), sd["pair_head"])
        b.step_pairs(img, cap, ig, cg)
        assert torch.equal(b.flat.params, a.flat.params) and torch.equal(b.pair_head.data, a.pair_head.data)
    plain = L.LoRATrainer(fresh()[3])
    sig = L.LoRAPairTrainer(fresh()[3], pair_loss="sigmoid")
    for other, name in ((plain, "infonce"), (sig, "sigmoid")):
        with pytest.raises(ValueError, match="with pair_loss='clip'"):
            other.load_state_dict(saved[False])
        with pytest.raises(ValueError, match=f"with pair_loss='{name}'"):
            b.load_state_dict(other.state_dict())


# ------------------------------------------------------------------------------------------- 7. two ranks
def _dp_step(dev, monkey, kind, rank=0, world=1):
    from clipfs import dist as D
    L, cfg, sd, model, layers, lw = TC._model(dev, monkey)
    B, M = (TC.DP_B, TC.DP_M) if kind == "groups" else (TC.DP_B, TC.DP_B)
    img, cap, ig, cg = TC._batch(cfg, kind, B, M)
    model.eval()
    tr = L.LoRAPairTrainer(model, logit_scale=30.0, pair_loss="clip", train_pair_head=True)
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
    for kind, collectives in (("paired", 5), ("groups", 6)):
        tr, (loss, c_it, c_ti) = _dp_step(dev, TC._Monkey, kind, rank, world)
        assert (tr.rank, tr.world) == (rank, world)
        assert tr.collectives_per_step == collectives, (kind, tr.collectives_per_step)
        tr.optimizer_step()  # the flat all-reduce: the ranks' shares of the head's gradient are summed with the rest
        total = torch.cat([loss, c_it.float(), c_ti.float()])
        D.allreduce_sum_(total)
        torch.cuda.synchronize()
        if rank == 0:
            np.savez(os.path.join(out_dir, f"clip_{kind}.npz"), grads=tr.flat.grads.cpu().numpy(), total=total.cpu().numpy())
    dist.destroy_process_group()


def test_two_ranks_match_one_process(dev, monkeypatch, tmp_path):
    """7 images on two ranks against 7 captions (pairs) and 5 captions (groups): a padding row in a gathered table either
    way.  5 collectives for plain pairs, 6 with groups (asserted on the ranks).  One process makes ONE symmetric call, a
    rank two one-directional ones."""
    want = {}
    for kind in ("paired", "groups"):
        tr, (loss, c_it, c_ti) = _dp_step(dev, monkeypatch, kind)
        assert tr.collectives_per_step == 0
        want[kind] = (tr.flat.grads.cpu().numpy(), loss.item(), c_it.item(), c_ti.item())
    mp.spawn(_pairs_rank, args=(2, TC._free_port(), str(tmp_path)), nprocs=2, join=True)
    for kind, (want_g, loss, hits_i, hits_t) in want.items():
        z = np.load(os.path.join(str(tmp_path), f"clip_{kind}.npz"))
        scale, hscale = np.abs(want_g[:-1]).max(), np.abs(want_g[-1])
        e_loss = abs(float(z["total"][0]) - loss)
        e_grad = np.abs(z["grads"][:-1] - want_g[:-1]).max() / scale
        e_head = np.abs(z["grads"][-1] - want_g[-1]) / hscale
        print(f"two ranks clip {kind}: loss {loss:.6f} err {e_loss:.3e} grad {e_grad:.3e} head {e_head:.3e} "
              f"hits {z['total'][1:]} / {hits_i} {hits_t}")
        assert scale > 1e-5 and hscale > 0
        assert e_loss <= TC.BOUND_DP_LOSS * max(1.0, abs(loss)) and e_grad <= TC.BOUND_DP_GRAD and e_head <= TC.BOUND_DP_GRAD
        assert (int(z["total"][1]), int(z["total"][2])) == (hits_i, hits_t)


# ------------------------------------------------------------------------------------------- 8. no host synchronisation
def test_step_pairs_does_not_synchronise(dev, monkeypatch):
    L, cfg, sd, model, layers, lw = TC._model(dev, monkeypatch, 0.25)
    img, cap, ig, cg = (t.to(dev) for t in TC._batch(cfg, "groups"))
    model.train()
    tr = L.LoRAPairTrainer(model, loss_scale=2.0 ** 12, max_grad_norm=1.0, pair_loss="clip", train_pair_head=True)
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
