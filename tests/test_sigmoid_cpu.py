"""Host-only checks of the sigmoid objective: the fp64 reference of the GPU tests against torch autograd of an
independently written formula (dhead included), the case table against the helper's conditions, the loss-scale factor,
clipfs_sigmoid_plan over the case table and every refusal of clipfs_sigmoid_objective (fake device addresses, a NULL
stream, nothing launched)."""
import ctypes

import pytest
import torch

from contrastive_ref import WIDE_GRAD, contrastive_inputs
from sigmoid_ref import CASES, REGIMES, head_of, sigmoid_case, sigmoid_loss, sigmoid_ref


@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("R,N,d,kind", [(1, 1, 64, "paired"), (32, 32, 64, "paired"), (33, 65, 64, "groups"),
                                        (37, 83, 192, "groups")])
def test_reference_is_the_autograd_of_the_definition(R, N, d, kind, regime):
    q, k, qg, kg = contrastive_inputs(R, N, d, kind)
    head = head_of(*REGIMES[regime])
    ref = sigmoid_ref(q, k, qg, kg, head, 1.0 / R)
    qd, kd, hd = (x.double().requires_grad_() for x in (q, k, head))
    loss = sigmoid_loss(qd, kd, qg, kg, hd, 1.0 / R)
    loss.backward()
    assert abs(loss.item() - ref["loss"].item()) <= 1e-12 * max(1.0, abs(loss.item()))
    for name, got in (("dq", qd.grad), ("dk", kd.grad), ("dhead", hd.grad)):
        assert (got - ref[name]).abs().max().item() <= 1e-12 * max(1.0, ref[name].abs().max().item()), name
    assert abs(ref["rows"][0].sum().item() / R - ref["loss"].item()) <= 1e-12 * max(1.0, ref["loss"].item())
    assert abs(ref["rows"][1].sum().item() / R - ref["dhead"][1].item()) <= 1e-12


def test_loss_scale_multiplies_the_gradients_only():
    q, k, qg, kg = contrastive_inputs(33, 65, 64, "groups")
    head = head_of(100.0, -10.0)
    a = sigmoid_ref(q, k, qg, kg, head, 0.25)
    b = sigmoid_ref(q, k, qg, kg, head, 0.25, scale=4096.0)
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["rows"], b["rows"]) and a["correct"] == b["correct"]
    for name in ("dq", "dk", "dhead"):
        assert torch.equal(a[name] * 4096.0, b[name]), name


def test_dead_cells_contribute_nothing_and_rows_without_a_positive_do():
    q, k, qg, kg = contrastive_inputs(37, 83, 192, "groups")
    head = head_of(100.0, -10.0)
    ref = sigmoid_ref(q, k, qg, kg, head, 1.0 / 37)
    keep = kg >= 0
    ref2 = sigmoid_ref(q, k[keep], qg, kg[keep], head, 1.0 / 37)  # dead keys: as if they were not there
    assert abs(ref["loss"].item() - ref2["loss"].item()) < 1e-12
    assert (ref["dq"] - ref2["dq"]).abs().max().item() < 1e-12 and (ref["dhead"] - ref2["dhead"]).abs().max().item() < 1e-12
    assert ref["dk"][~keep].abs().max().item() == 0 and ref["dq"][qg < 0].abs().max().item() == 0
    assert bool((ref["rows"][:3, qg < 0] == 0).all()) and bool((ref["rows"][3, qg < 0] == -1).all())
    kg2 = kg.clone()
    kg2[kg2 == qg[qg >= 0][0]] = 10 ** 6  # the first live query loses its positives: its row still pays
    i = int((qg >= 0).nonzero()[0])
    ref3 = sigmoid_ref(q, k, qg, kg2, head, 1.0 / 37)
    assert ref3["rows"][0, i].item() > 0 and ref3["dq"][i].abs().max().item() > 0


@pytest.mark.parametrize("regime", list(REGIMES))
def test_case_table_satisfies_the_helper_conditions(regime):
    for case in CASES:
        sigmoid_case(*case, regime)


@pytest.fixture(scope="module")
def lib():
    from clipfs import _lib
    return _lib.load()


BENCH_SHAPES = [(256, 256, 512), (256, 403, 512), (512, 4096, 512), (256, 2048, 1024)]


@pytest.mark.parametrize("R,N,d", [c[:3] for c in CASES] + BENCH_SHAPES + [(8192, 8192, 1024), (1, 70000, 4)])
def test_plan_covers_the_shape(R, N, d):
    from clipfs import ops
    plans = {op: ops.sigmoid_plan(op, R, N, d) for op in ("rows", "combine", "dq", "dk")}
    assert plans["rows"]["grid"] == (-(-R // 32), 1, 1) and plans["rows"]["feat_chunk"] == 0
    assert plans["combine"]["grid"] == (1, 1, 1) and plans["combine"]["feat_chunk"] == 0
    for op, own in (("dq", R), ("dk", N)):
        p = plans[op]
        assert p["feat_chunk"] in (128, 512)
        assert p["grid"] == (-(-own // 32), -(-d // p["feat_chunk"]), 1)
        assert p["grid"][0] * 32 >= own and p["grid"][1] * p["feat_chunk"] >= d
    for p in plans.values():
        assert p["block"] == 256 and 0 < p["lds_bytes"] <= 160 * 1024
        assert sorted(p) == ["block", "feat_chunk", "grid", "lds_bytes"]  # no scratch size: the entry point takes none


@pytest.mark.parametrize("case,op", WIDE_GRAD)
def test_wide_gradient_cases_reach_the_512_feature_workgroups(case, op):
    from clipfs import ops
    assert case in CASES
    R, N, d, _ = case
    other = "dk" if op == "dq" else "dq"
    assert ops.sigmoid_plan(op, R, N, d)["feat_chunk"] == 512
    assert ops.sigmoid_plan(other, R, N, d)["feat_chunk"] == 128


def test_plan_refusals():
    from clipfs import _lib, ops
    for args, word in (((0, 4, 64), "R = 0"), ((4, 0, 64), "N = 0"), ((4, 4, 0), "d = 0"), ((4, 4, 6), "d = 6"),
                       ((4, 4, 1028), "d = 1028")):
        with pytest.raises(_lib.ClipfsError, match=word):
            ops.sigmoid_plan("rows", *args)
    assert _lib.load().clipfs_sigmoid_plan(0, 4, 4, 64, None) == 1 and b"NULL plan" in _lib.load().clipfs_last_error()
    plan = _lib.SigmoidPlan()
    assert _lib.load().clipfs_sigmoid_plan(4, 4, 4, 64, ctypes.byref(plan)) == 1
    assert b"unknown op 4" in _lib.load().clipfs_last_error() and plan.block == 0  # nothing written on refusal


def test_objective_refuses_before_launching(lib):
    """Every refusal returns CLIPFS_EINVAL with the argument named; the addresses are never dereferenced."""
    q, k, qg, kg, head, rows, lsum, cor, dq, dk, dhead, state = (0x100000 * (i + 1) for i in range(12))

    def call(q=q, k=k, qg=qg, kg=kg, head=head, rows=rows, lsum=lsum, dq=dq, dk=dk, dhead=dhead, R=8, N=12, d=64, w=1.0,
             state=None):
        return lib.clipfs_sigmoid_objective(q, k, qg, kg, head, w, state, rows, lsum, cor, dq, 0, dk, 1, dhead, 0, R, N, d, None)

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
    refused(call(rows=None), b"row_stats is NULL")
    refused(call(lsum=None), b"loss_sum is NULL")
    refused(call(q=q + 4), b"q is NULL or not 16-byte")
    refused(call(k=k + 8), b"k is NULL or not 16-byte")
    refused(call(dq=dq + 4), b"dq is not 16-byte")
    refused(call(dk=dk + 12), b"dk is not 16-byte")
    refused(call(dq=q), b"dq aliases q or k")
    refused(call(dq=k), b"dq aliases q or k")
    refused(call(dk=k), b"dk aliases q or k")
    refused(call(dk=q + 16), b"dk aliases q or k")  # an overlap, not only the same base
    refused(call(dq=dk), b"dq aliases dk")
    refused(call(head=q + 4), b"head aliases q or k")
    refused(call(head=k + 8 * 12 - 4), b"head aliases q or k")
    refused(call(head=dq + 4), b"head aliases dq or dk")
    refused(call(head=dk), b"head aliases dq or dk")
    refused(call(dhead=q), b"dhead aliases q or k")
    refused(call(dhead=k + 4), b"dhead aliases q or k")
    refused(call(dhead=dq), b"dhead aliases dq or dk")
    refused(call(dhead=dk + 4), b"dhead aliases dq or dk")
    refused(call(dhead=head + 4), b"dhead aliases head")
    refused(call(w=float("-inf")), b"weight")
    refused(call(w=float("nan")), b"weight")
    refused(call(state=state + 4), b"scaler_state")


def test_ops_wrapper_refuses_cpu_tensors_and_a_bad_head():
    from clipfs import ops
    q, k, qg, kg = contrastive_inputs(4, 4, 8, "paired")
    head = head_of(10.0, -10.0)
    with pytest.raises(AssertionError):
        ops.sigmoid_objective(q, k, qg.long(), kg, head)
    with pytest.raises(AssertionError, match="two contiguous floats"):
        ops.sigmoid_objective(q, k, qg, kg, torch.zeros(3))
    with pytest.raises(AssertionError, match="two contiguous floats"):
        ops.sigmoid_objective(q, k, qg, kg, head.double())
    with pytest.raises(AssertionError, match="device tensors"):
        ops.sigmoid_objective(q, k, qg, kg, head)
    with pytest.raises(ValueError, match="3 images, 4 captions"):
        ops.siglip_loss(q[:3], k, head=head)
    with pytest.raises(ValueError, match="both img_group and txt_group"):
        ops.siglip_loss(q, k, img_group=qg, head=head)
