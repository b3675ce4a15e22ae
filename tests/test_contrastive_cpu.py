"""Host-only checks of the contrastive objective: the fp64 reference of the GPU tests against torch autograd of an
independently written formula, the paired special case, the key mask, clipfs_contrastive_plan over the case table and
every refusal of clipfs_contrastive_objective (fake device addresses, a NULL stream, nothing launched)."""
import pytest
import torch

from contrastive_ref import CASES, WIDE_GRAD, contrastive_case, contrastive_inputs, contrastive_ref


def _autograd(q, k, qg, kg, s, w):
    """The definition row by row with python loops and autograd: nothing shared with contrastive_ref."""
    q = q.double().clone().requires_grad_()
    k = k.double().clone().requires_grad_()
    total = torch.zeros((), dtype=torch.float64)
    rows = []
    for i in range(q.shape[0]):
        livej = [j for j in range(k.shape[0]) if int(kg[j]) >= 0]
        posj = [j for j in livej if int(kg[j]) == int(qg[i])]
        if int(qg[i]) < 0 or not posj:
            rows.append(0.0)
            continue
        z = s * (k[livej] @ q[i])
        zp = s * (k[posj] @ q[i])
        li = torch.log(torch.exp(z - z.max().detach()).sum()) + z.max().detach() - zp.mean()
        rows.append(float(li.detach()))
        total = total + li
    (w * total).backward()
    return float((w * total).detach()), torch.tensor(rows, dtype=torch.float64), q.grad, k.grad


@pytest.mark.parametrize("R,N,d,kind", [c for c in CASES if c[0] * c[1] <= 37 * 83] + [(40, 24, 32, "groups")])
@pytest.mark.parametrize("s", [100.0, 1.0])
def test_reference_is_the_autograd_of_the_definition(R, N, d, kind, s):
    q, k, qg, kg = contrastive_inputs(R, N, d, kind)
    ref = contrastive_ref(q, k, qg, kg, s, 1.0 / R)
    loss, rows, dq, dk = _autograd(q, k, qg, kg, s, 1.0 / R)
    assert abs(float(ref["loss"]) - loss) < 1e-12 * max(1.0, abs(loss))
    assert (ref["loss_rows"] - rows).abs().max().item() < 1e-11
    assert (ref["dq"] - dq).abs().max().item() < 1e-12 * s
    assert (ref["dk"] - dk).abs().max().item() < 1e-12 * s


def test_loss_scale_multiplies_the_gradients_only():
    q, k, qg, kg = contrastive_inputs(33, 65, 64, "groups")
    a = contrastive_ref(q, k, qg, kg, 100.0, 0.25)
    b = contrastive_ref(q, k, qg, kg, 100.0, 0.25, scale=4096.0)
    assert float(a["loss"]) == float(b["loss"]) and a["correct"] == b["correct"]
    assert torch.equal(a["dq"] * 4096.0, b["dq"]) and torch.equal(a["dk"] * 4096.0, b["dk"])


@pytest.mark.parametrize("n,d", [(32, 64), (256, 512)])
def test_paired_case_is_the_symmetric_cross_entropy(n, d):
    q, k, qg, kg = contrastive_inputs(n, n, d, "paired")
    z = 100.0 * q.double() @ k.double().t()
    tgt = torch.arange(n)
    ce = 0.5 * (torch.nn.functional.cross_entropy(z, tgt) + torch.nn.functional.cross_entropy(z.t(), tgt))
    i2t = contrastive_ref(q, k, qg, kg, 100.0, 0.5 / n)
    t2i = contrastive_ref(k, q, kg, qg, 100.0, 0.5 / n)
    assert abs(float(i2t["loss"] + t2i["loss"]) - float(ce)) < 1e-12 * float(ce)
    assert i2t["correct"] == int((z.argmax(1) == tgt).sum()) and t2i["correct"] == int((z.argmax(0) == tgt).sum())


def test_a_masked_key_changes_nothing_but_its_own_column():
    q, k, qg, kg = contrastive_inputs(37, 83, 192, "groups")
    dead = int((kg < 0).nonzero()[0])
    ref = contrastive_ref(q, k, qg, kg, 100.0, 1.0 / 37)
    k2 = k.clone()
    k2[dead] = -k2[dead] + 0.5  # any other row: not even a unit one
    ref2 = contrastive_ref(q, k2, qg, kg, 100.0, 1.0 / 37)
    keep = torch.arange(83) != dead
    assert torch.equal(ref["loss_rows"], ref2["loss_rows"]) and ref["correct"] == ref2["correct"]
    assert torch.equal(ref["dq"], ref2["dq"]) and torch.equal(ref["dk"][keep], ref2["dk"][keep])
    assert ref["dk"][dead].abs().max().item() == 0 and ref2["dk"][dead].abs().max().item() == 0
    # ... and dropping the masked keys altogether gives the same rows
    ref3 = contrastive_ref(q, k[kg >= 0], qg, kg[kg >= 0], 100.0, 1.0 / 37)
    assert (ref["loss_rows"] - ref3["loss_rows"]).abs().max().item() < 1e-12
    assert (ref["dq"] - ref3["dq"]).abs().max().item() < 1e-12


@pytest.mark.parametrize("s", [100.0, 1.0])
def test_case_table_satisfies_the_helper_conditions(s):
    for case in CASES:
        contrastive_case(*case, s)


@pytest.fixture(scope="module")
def lib():
    from clipfs import _lib
    return _lib.load()


BENCH_SHAPES = [(256, 256, 512), (256, 403, 512), (512, 4096, 512), (256, 2048, 1024)]


@pytest.mark.parametrize("R,N,d", [c[:3] for c in CASES] + BENCH_SHAPES + [(8192, 8192, 1024), (1, 70000, 4)])
def test_plan_covers_the_shape(R, N, d):
    from clipfs import ops
    plans = {op: ops.contrastive_plan(op, R, N, d) for op in ("stats", "combine", "dq", "dk")}
    st = plans["stats"]
    assert st["col_chunk"] % 128 == 0 and 128 <= st["col_chunk"] <= 1024
    assert st["chunks"] == -(-N // st["col_chunk"])
    assert st["grid"] == (-(-R // 32), st["chunks"], 1)
    assert plans["combine"]["grid"] == (1, 1, 1)
    for op, own in (("dq", R), ("dk", N)):
        p = plans[op]
        assert p["feat_chunk"] in (128, 512)
        assert p["grid"] == (-(-own // 32), -(-d // p["feat_chunk"]), 1)
        assert p["grid"][0] * 32 >= own and p["grid"][1] * p["feat_chunk"] >= d
    for p in plans.values():
        assert p["block"] == 256 and 0 < p["lds_bytes"] <= 160 * 1024
        assert p["work_floats"] == 6 * st["chunks"] * R + 2 * R
        assert (p["col_chunk"], p["chunks"]) == (st["col_chunk"], st["chunks"])


@pytest.mark.parametrize("case,op", WIDE_GRAD)
def test_wide_gradient_cases_reach_the_512_feature_workgroups(case, op):
    """The two cases that exist to run the four-accumulator gradient kernels must keep selecting them."""
    from clipfs import ops
    assert case in CASES
    R, N, d, _ = case
    other = "dk" if op == "dq" else "dq"
    assert ops.contrastive_plan(op, R, N, d)["feat_chunk"] == 512
    assert ops.contrastive_plan(other, R, N, d)["feat_chunk"] == 128


def test_plan_refusals():
    from clipfs import _lib, ops
    for args, word in (((0, 4, 64), "R = 0"), ((4, 0, 64), "N = 0"), ((4, 4, 0), "d = 0"), ((4, 4, 6), "d = 6"),
                       ((4, 4, 1028), "d = 1028")):
        with pytest.raises(_lib.ClipfsError, match=word):
            ops.contrastive_plan("stats", *args)
    assert _lib.load().clipfs_contrastive_plan(0, 4, 4, 64, None) == 1 and b"NULL plan" in _lib.load().clipfs_last_error()
    plan = _lib.ContrastivePlan()
    import ctypes
    assert _lib.load().clipfs_contrastive_plan(4, 4, 4, 64, ctypes.byref(plan)) == 1
    assert b"unknown op 4" in _lib.load().clipfs_last_error() and plan.block == 0  # nothing written on refusal


def test_objective_refuses_before_launching(lib):
    """Every refusal returns CLIPFS_EINVAL with the argument named; the addresses are never dereferenced."""
    q, k, qg, kg, rows, lsum, cor, dq, dk, work, state = (0x100000 * (i + 1) for i in range(11))

    def call(q=q, k=k, qg=qg, kg=kg, lsum=lsum, dq=dq, dk=dk, work=work, R=8, N=12, d=64, s=100.0, w=1.0, state=None):
        return lib.clipfs_contrastive_objective(q, k, qg, kg, s, w, state, rows, lsum, cor, dq, 0, dk, 1, work, R, N, d, None)

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
    refused(call(lsum=None), b"loss_sum is NULL")
    refused(call(work=None), b"work is NULL")
    refused(call(q=q + 4), b"q is NULL or not 16-byte")
    refused(call(k=k + 8), b"k is NULL or not 16-byte")
    refused(call(dq=dq + 4), b"dq is not 16-byte")
    refused(call(dk=dk + 12), b"dk is not 16-byte")
    refused(call(dq=q), b"dq aliases q or k")
    refused(call(dq=k), b"dq aliases q or k")
    refused(call(dk=k), b"dk aliases q or k")
    refused(call(dk=q + 16), b"dk aliases q or k")  # an overlap, not only the same base
    refused(call(dq=dk), b"dq aliases dk")
    refused(call(s=float("inf")), b"logit_scale")
    refused(call(s=float("nan")), b"logit_scale")
    refused(call(w=float("-inf")), b"weight")
    refused(call(w=float("nan")), b"weight")
    refused(call(state=state + 4), b"scaler_state")


def test_ops_wrapper_refuses_cpu_tensors_and_bad_groups():
    from clipfs import ops
    q, k, qg, kg = contrastive_inputs(4, 4, 8, "paired")
    with pytest.raises(AssertionError):
        ops.contrastive_objective(q, k, qg.long(), kg)
    with pytest.raises(AssertionError, match="device tensors"):
        ops.contrastive_objective(q, k, qg, kg)
    with pytest.raises(ValueError, match="3 images, 4 captions"):
        ops.clip_loss(q[:3], k)
    with pytest.raises(ValueError, match="both img_group and txt_group"):
        ops.clip_loss(q, k, img_group=qg)
