"""Host-only checks of the symmetric CLIP pair objective and the AdamW tail: the closed-form dhead of the reference against
fp64 autograd of contrastive_ref.symmetric_loss with respect to log s, the case table against the helper's conditions and
the arg-max rule, clipfs_clip_pairs_plan, every refusal of clipfs_clip_pairs_objective and clipfs_adamw_tail (fake device
addresses, a NULL stream, nothing launched), and the constructor of LoRAPairTrainer's refusals that need no model."""
import ctypes

import pytest
import torch

from clip_pairs_ref import CASES, GAP, ONE_DIRECTIONAL, PEAKED, SCALES, clip_pairs_case, clip_pairs_ref, head_of
from contrastive_ref import WIDE_GRAD, contrastive_inputs, symmetric_loss


@pytest.mark.parametrize("s", [100.0, 1.0 / 0.07, 1.0])
@pytest.mark.parametrize("R,N,d,kind", [(1, 1, 64, "paired"), (32, 32, 64, "paired"), (33, 65, 64, "groups"),
                                        (37, 83, 192, "groups"), (300, 40, 128, "groups")])
def test_dhead_is_the_autograd_of_the_symmetric_loss_in_log_s(R, N, d, kind, s):
    q, k, qg, kg = contrastive_inputs(R, N, d, kind)
    head = head_of(s)
    ref = clip_pairs_ref(q, k, qg, kg, head, 0.5 / R, 0.5 / N)
    qd, kd, hd = q.double().requires_grad_(), k.double().requires_grad_(), head.double().requires_grad_()
    loss = symmetric_loss(qd, kd, qg, kg, torch.exp(hd[0]))
    loss.backward()
    tol = lambda x: 1e-12 * max(1.0, float(x.abs().max()))
    assert abs(loss.item() - float(ref["loss"])) <= tol(loss)
    assert abs(hd.grad.item() - float(ref["dhead"])) <= 1e-12 * max(1.0, float(ref["dhead_scale"]))
    assert float((qd.grad - ref["dq"]).abs().max()) <= tol(ref["dq"]) and float((kd.grad - ref["dk"]).abs().max()) <= tol(ref["dk"])
    # the row statistic is the row's share: w sum_i (E[z] - mean_P z) = that direction's dhead
    for side, w in ((ref["qside"], 0.5 / R), (ref["kside"], 0.5 / N)):
        assert abs(w * float(side["rows"][3].sum()) - float(side["dhead"])) <= 1e-12 * max(1.0, float(side["dhead_scale"]))


def test_one_directional_reference_and_loss_scale():
    q, k, qg, kg = contrastive_inputs(33, 65, 64, "groups")
    head = head_of(100.0)
    one = clip_pairs_ref(q, k, qg, kg, head, 1.0 / 33)
    assert one["kside"] is None and one["correct"][1] == 0
    two = clip_pairs_ref(q, k, qg, kg, head, 1.0 / 33, 1.0 / 65)
    swapped = clip_pairs_ref(k, q, kg, qg, head, 1.0 / 65)
    assert torch.equal(two["loss"], one["loss"] + swapped["loss"]) and torch.equal(two["dq"], one["dq"] + swapped["dk"])
    assert torch.equal(two["dhead"], one["dhead"] + swapped["dhead"])
    scaled = clip_pairs_ref(q, k, qg, kg, head, 1.0 / 33, 1.0 / 65, scale=4096.0)
    assert torch.equal(scaled["loss"], two["loss"])
    for name in ("dq", "dk", "dhead"):
        assert torch.equal(scaled[name], two[name] * 4096.0), name


@pytest.mark.parametrize("name", list(SCALES))
def test_case_table_is_honest_in_both_directions(name):
    """The helper's conditions hold for every case in both directions, and the arg-max rule has something to stand on:
    rows whose own top-1 / top-2 gap is below GAP s are at most 1 % of a direction's rows."""
    s = SCALES[name]
    tight = []
    for case in CASES:
        *_, ref, _ = clip_pairs_case(*case, s)
        for tag, side in (("q", ref["qside"]), ("k", ref["kside"])):
            close = int((side["gaps"] < GAP * s).sum())
            assert close * 100 <= len(side["gaps"]), (case, tag, close)
            if close:
                tight.append((case, tag, close, float(side["gaps"].min()) / s))
    print(f"s = {name}: directions with a gap below {GAP} s:", tight)
    assert len(tight) <= 1  # (40, 4081, 600): its 4081-row direction
    for case in ONE_DIRECTIONAL:
        clip_pairs_case(*case, s, both=False)


def test_peaked_case_is_peaked():
    case, s = PEAKED
    q, k, qg, kg, _, ref, _ = clip_pairs_case(*case, s, honest=False)
    alive = ref["qside"]["alive"]
    # the best key holds most of the softmax on most rows that count: lse - z_best < log 2
    z = ref["s"] * q.double() @ k.double().t()
    z = z.masked_fill((kg < 0)[None, :], float("-inf"))
    share = torch.exp(z.max(1).values - torch.logsumexp(z, 1))[alive]
    assert float((share > 0.5).double().mean()) >= 0.75, float((share > 0.5).double().mean())


# ------------------------------------------------------------------------------------------- the plan
BENCH_SHAPES = [(256, 256, 512), (256, 403, 512), (512, 4096, 512), (256, 2048, 1024)]


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("R,N,d", [c[:3] for c in CASES] + BENCH_SHAPES + [(8192, 8192, 1024), (1, 70000, 4)])
def test_plan_covers_the_shape(R, N, d, both):
    from clipfs import ops
    plans = {op: ops.clip_pairs_plan(op, R, N, d, both) for op in ("rows", "combine", "dq", "dk")}
    assert plans["rows"]["grid"] == (-(-R // 32) + (-(-N // 32) if both else 0), 1, 1) and plans["rows"]["feat_chunk"] == 0
    assert plans["combine"]["grid"] == (1, 1, 1) and plans["combine"]["feat_chunk"] == 0
    for op, own in (("dq", R), ("dk", N)):
        p = plans[op]
        assert p["feat_chunk"] in (128, 512)
        assert p["grid"] == (-(-own // 32), -(-d // p["feat_chunk"]), 1)
    for p in plans.values():
        assert p["block"] == 256 and 0 < p["lds_bytes"] <= 64 * 1024
        assert sorted(p) == ["block", "feat_chunk", "grid", "lds_bytes"]  # no scratch size: the entry point takes none


@pytest.mark.parametrize("case,op", WIDE_GRAD)
def test_wide_gradient_cases_plan_512_features(case, op):
    from clipfs import ops
    assert case in CASES
    R, N, d, _ = case
    other = "dk" if op == "dq" else "dq"
    assert ops.clip_pairs_plan(op, R, N, d)["feat_chunk"] == 512
    assert ops.clip_pairs_plan(other, R, N, d)["feat_chunk"] == 128


def test_plan_refusals():
    from clipfs import _lib, ops
    for args, word in (((0, 4, 64), "R = 0"), ((4, 0, 64), "N = 0"), ((4, 4, 0), "d = 0"), ((4, 4, 6), "d = 6"),
                       ((4, 4, 1028), "d = 1028")):
        with pytest.raises(_lib.ClipfsError, match=word):
            ops.clip_pairs_plan("rows", *args)
    lib = _lib.load()
    assert lib.clipfs_clip_pairs_plan(0, 4, 4, 64, 1, None) == 1 and b"NULL plan" in lib.clipfs_last_error()
    plan = _lib.ClipPairsPlan()
    assert lib.clipfs_clip_pairs_plan(4, 4, 4, 64, 1, ctypes.byref(plan)) == 1
    assert b"unknown op 4" in lib.clipfs_last_error() and plan.block == 0  # nothing written on refusal
    assert lib.clipfs_clip_pairs_plan(0, 4, 4, 64, 2, ctypes.byref(plan)) == 1 and b"both = 2" in lib.clipfs_last_error()


def test_symbols_are_bound():
    from clipfs import _lib
    for name in ("clipfs_adamw_tail", "clipfs_clip_pairs_plan", "clipfs_clip_pairs_objective"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)


@pytest.fixture(scope="module")
def lib():
    from clipfs import _lib
    return _lib.load()


def test_objective_refuses_before_launching(lib):
    """Every refusal returns CLIPFS_EINVAL with the argument named; the addresses are never dereferenced."""
    q, k, qg, kg, head, qs, ks, lsum, cor, dq, dk, dhead, state = (0x100000 * (i + 1) for i in range(13))

    def call(q=q, k=k, qg=qg, kg=kg, head=head, qs=qs, ks=ks, lsum=lsum, dq=dq, dk=dk, dhead=dhead, R=8, N=12, d=64, wq=1.0,
             wk=0.5, state=None):
        return lib.clipfs_clip_pairs_objective(q, k, qg, kg, head, wq, wk, state, qs, ks, lsum, cor, dq, 0, dk, 1, dhead, 0, R, N,
                                               d, None)

    def refused(rc, word):
        assert rc == 1 and word in lib.clipfs_last_error(), (rc, lib.clipfs_last_error())

    refused(call(R=0), b"R = 0")
    refused(call(N=-1), b"N = -1")
    refused(call(d=0), b"d = 0")
    refused(call(d=66), b"d = 66")
    refused(call(d=1028), b"d = 1028")
    refused(call(q=None), b"q is NULL")
    refused(call(k=None), b"k is NULL")
    refused(call(qg=None), b"q_group is NULL")
    refused(call(kg=None), b"k_group is NULL")
    refused(call(head=None), b"head is NULL")
    refused(call(qs=None), b"q_stats is NULL")
    refused(call(lsum=None), b"loss_sum is NULL")
    refused(call(ks=None), b"k_stats is NULL with weight_k != 0")
    refused(call(wk=0.0), b"k_stats must be NULL when weight_k == 0")
    refused(call(q=q + 4), b"q is NULL or not 16-byte")
    refused(call(k=k + 8), b"k is NULL or not 16-byte")
    refused(call(dq=dq + 4), b"dq is not 16-byte")
    refused(call(dk=dk + 12), b"dk is not 16-byte")
    refused(call(dq=q), b"dq aliases q or k")
    refused(call(dk=q + 16), b"dk aliases q or k")  # an overlap, not only the same base
    refused(call(dq=dk), b"dq aliases dk")
    refused(call(head=q + 4), b"head aliases q or k")
    refused(call(head=dk), b"head aliases dq or dk")
    refused(call(dhead=k + 4), b"dhead aliases q or k")
    refused(call(dhead=dq), b"dhead aliases dq or dk")
    refused(call(dhead=head), b"dhead aliases head")
    refused(call(qs=q), b"q_stats aliases")
    refused(call(qs=dk + 4), b"q_stats aliases")
    refused(call(ks=qs + 4 * 8), b"k_stats aliases")
    refused(call(ks=head - 4), b"k_stats aliases")
    refused(call(wq=float("-inf")), b"weight_q")
    refused(call(wk=float("nan")), b"weight_k")
    refused(call(state=state + 4), b"scaler_state")


def test_adamw_tail_refuses_before_launching(lib):
    p, g, m, v, sh = (0x100000 * (i + 1) for i in range(5))
    inf = float("inf")

    def call(n=16, step=1, tail_n=2, lo=-inf, hi=inf, shadow=None, decay=0.0):
        return lib.clipfs_adamw_tail(p, g, m, v, n, step, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1.0, None, None, shadow, decay, tail_n,
                                     0.0, lo, hi, None)

    def refused(rc, word):
        assert rc == 1 and word in lib.clipfs_last_error(), (rc, lib.clipfs_last_error())

    refused(call(tail_n=17), b"tail_n = 17 exceeds n = 16")
    refused(call(lo=1.0, hi=0.5), b"tail_min = 1 exceeds tail_max = 0.5")
    refused(call(lo=float("nan")), b"is NaN")
    refused(call(hi=float("nan")), b"is NaN")
    refused(call(n=0, tail_n=0), b"n = 0")
    refused(call(step=0), b"step 0 must be >= 1")
    refused(call(shadow=p, decay=0.5), b"aliased ema shadow")
    refused(call(shadow=sh, decay=1.0), b"ema_decay")


def test_ops_wrapper_refuses_cpu_tensors_and_a_bad_head():
    from clipfs import ops
    q, k, qg, kg = contrastive_inputs(4, 4, 8, "paired")
    head = head_of(100.0)
    with pytest.raises(AssertionError):
        ops.clip_pairs_objective(q, k, qg.long(), kg, head, 1.0)
    with pytest.raises(AssertionError, match="one float"):
        ops.clip_pairs_objective(q, k, qg, kg, torch.zeros(2), 1.0)
    with pytest.raises(AssertionError, match="one float"):
        ops.clip_pairs_objective(q, k, qg, kg, head.double(), 1.0)
    with pytest.raises(AssertionError, match="device tensors"):
        ops.clip_pairs_objective(q, k, qg, kg, head, 1.0)
    with pytest.raises(ValueError, match="3 images, 4 captions"):
        ops.clip_pairs_loss(q[:3], k, head=head)
    with pytest.raises(ValueError, match="both img_group and txt_group"):
        ops.clip_pairs_loss(q, k, img_group=qg, head=head)


def test_pair_trainer_refusals_that_need_no_model():
    import lora_train_vlp as L
    new = lambda **kw: L.LoRAPairTrainer(None, **kw)
    with pytest.raises(ValueError, match="pair_loss must be"):
        new(pair_loss="hinge")
    with pytest.raises(ValueError, match="train_pair_head needs"):
        new(train_pair_head=True)
    with pytest.raises(ValueError, match="pair_scale belongs to pair_loss='sigmoid'"):
        new(pair_loss="clip", pair_scale=20.0)
    with pytest.raises(ValueError, match="pair_bias belongs to pair_loss='sigmoid'"):
        new(pair_loss="clip", pair_bias=0.0)
    with pytest.raises(ValueError, match="pair_scale_max needs pair_loss='clip'"):
        new(pair_loss="sigmoid", pair_scale_max=50.0)
    with pytest.raises(ValueError, match="pair_scale_max needs pair_loss='clip'"):
        new(pair_scale_max=None)
    with pytest.raises(ValueError, match="pair_scale_max must be"):
        new(pair_loss="clip", pair_scale_max=0.0)
    with pytest.raises(ValueError, match="pair_head_weight_decay must be"):
        new(pair_loss="clip", pair_head_weight_decay=-1.0)
    with pytest.raises(ValueError, match="logit_scale must be a positive"):
        new(pair_loss="clip", logit_scale=0.0)
