"""clipfs_spd_*_panels and clipfs_krr_* without a GPU: every refusal names its argument before anything is enqueued (no
device is opened: the fake, aligned addresses handed over are never dereferenced) and nothing is written on refusal."""
import ctypes as C

import numpy as np
import pytest

from clipfs import _lib, ops

A0, A1, A2, A3, A4, A5, A6 = (k << 32 for k in range(1, 8))  # fake, aligned, far apart


def _err(rc):
    return rc, _lib.load().clipfs_last_error()


# ------------------------------------------------------------------------------------------------------- SPD panels
@pytest.mark.parametrize("n,nrhs,panel,name", [(0, 1, 256, "n"), (6, 1, 256, "n"), (16388, 1, 256, "n"), (64, 0, 256, "nrhs"),
                                               (64, 65537, 256, "nrhs"), (64, 1, 0, "panel"), (64, 1, 48, "panel"),
                                               (64, 1, 1056, "panel"), (64, 1, -32, "panel")])
def test_panels_plan_refusals(n, nrhs, panel, name):
    lib = _lib.load()
    plan = _lib.SpdPanelsPlan()
    plan.panel = -7
    rc, msg = _err(lib.clipfs_spd_panels_plan(n, nrhs, panel, C.byref(plan)))
    assert rc == 1 and f" {name} = ".encode() in msg, msg
    assert plan.panel == -7  # nothing written on refusal
    with pytest.raises(_lib.ClipfsError):
        ops.spd_panels_plan(n, nrhs, panel)
    rc, msg = _err(lib.clipfs_spd_panels_plan(64, 1, 64, None))
    assert rc == 1 and b"plan" in msg


def _factor(A=A0, lda=2048, L=A1, ldl=2048, n=2048, panel=256, info=A2):
    return _err(_lib.load().clipfs_spd_factor_panels(A, lda, L, ldl, n, panel, info, None))


FACTOR_REFUSALS = [
    (dict(n=6), " n = "), (dict(n=16388, lda=16388, ldl=16388), " n = "), (dict(panel=40), " panel = "), (dict(panel=2048), " panel = "),
    (dict(A=None), " A is NULL"), (dict(L=None), " L is NULL"), (dict(info=None), " info is NULL"),
    (dict(A=A0 + 4), " A is not 16-byte aligned"), (dict(L=A1 + 8), " L is not 16-byte aligned"),
    (dict(info=A2 + 2), " info is not 4-byte aligned"), (dict(lda=2044), " lda = "), (dict(lda=2050), " lda = "), (dict(ldl=32), " ldl = "),
    (dict(L=A0, ldl=2056), " L overlaps A"), (dict(L=A0 + 64), " L overlaps A"), (dict(info=A0 + 16), " info overlaps"),
    (dict(info=A1 + 4 * (2047 * 2048 + 2047)), " info overlaps"),
]


@pytest.mark.parametrize("over,text", FACTOR_REFUSALS, ids=[f"{i}" for i in range(len(FACTOR_REFUSALS))])
def test_factor_panels_refusals(over, text):
    rc, msg = _factor(**over)
    assert rc == 1 and text.encode() in msg and b"clipfs_spd_factor_panels" in msg, msg


def _solve(L=A0, ldl=2048, n=2048, panel=256, R=A1, ldr=2048, X=A2, ldx=2048, nrhs=70, alpha=1.0):
    return _err(_lib.load().clipfs_spd_solve_panels(L, ldl, n, panel, R, ldr, X, ldx, nrhs, alpha, None))


SOLVE_REFUSALS = [
    (dict(n=2), " n = "), (dict(panel=100), " panel = "), (dict(nrhs=0), " nrhs = "), (dict(nrhs=65537), " nrhs = "),
    (dict(L=None), " L is NULL"), (dict(R=None), " R is NULL"), (dict(X=None), " X is NULL"),
    (dict(R=A1 + 4), " R is not 16-byte aligned"), (dict(X=A2 + 4), " X is not 16-byte aligned"), (dict(ldr=2046), " ldr = "),
    (dict(ldx=2040), " ldx = "), (dict(ldl=2047), " ldl = "), (dict(alpha=float("nan")), " alpha = "),
    (dict(alpha=float("inf")), " alpha = "), (dict(X=A1, ldx=4096), " X overlaps R"), (dict(X=A1 + 256), " X overlaps R"),
    (dict(X=A0 + 16), " X overlaps L"),
]


@pytest.mark.parametrize("over,text", SOLVE_REFUSALS, ids=[f"{i}" for i in range(len(SOLVE_REFUSALS))])
def test_solve_panels_refusals(over, text):
    rc, msg = _solve(**over)
    assert rc == 1 and text.encode() in msg and b"clipfs_spd_solve_panels" in msg, msg


# ---------------------------------------------------------------------------------------------------------------- KRR
@pytest.mark.parametrize("over,name", [(dict(d=130), "d"), (dict(d=0), "d"), (dict(d=1028), "d"), (dict(n=0), "n"), (dict(n=16385), "n"),
                                       (dict(C=0), "C"), (dict(C=4097), "C"), (dict(B=0), "B"), (dict(panel=48), "panel"),
                                       (dict(n=2000, panel=48), "panel"), (dict(panel=2048), "panel")])
def test_krr_plan_refusals(over, name):
    lib = _lib.load()
    a = {**dict(n=132, C=37, d=64, B=70, panel=256), **over}
    plan = _lib.KrrPlan()
    plan.n4 = -7
    rc, msg = _err(lib.clipfs_krr_plan(a["n"], a["C"], a["d"], a["B"], a["panel"], C.byref(plan)))
    assert rc == 1 and f" {name} = ".encode() in msg, msg
    assert plan.n4 == -7
    with pytest.raises(_lib.ClipfsError):
        ops.krr_plan(a["n"], a["C"], a["d"], a["B"], a["panel"])
    assert lib.clipfs_krr_plan(132, 37, 64, 70, 256, None) == 1 and b"plan" in lib.clipfs_last_error()


def _system(S=A0, A=A1, n=130, d=64, ld=132, beta=5.5, lam=1.0):
    return _err(_lib.load().clipfs_krr_system(S, A, n, d, ld, beta, lam, None))


SYSTEM_REFUSALS = [
    (dict(d=66), " d = "), (dict(n=0), " n = "), (dict(n=16385, ld=16388), " n = "), (dict(beta=0.0), " beta = "), (dict(beta=100.5), " beta = "),
    (dict(beta=float("nan")), " beta = "), (dict(lam=0.0), " lambda = "), (dict(lam=-1.0), " lambda = "), (dict(lam=float("inf")), " lambda = "),
    (dict(ld=128), " ld = "), (dict(ld=134), " ld = "), (dict(S=None), " S is NULL"), (dict(A=None), " A is NULL"),
    (dict(S=A0 + 4), " S is not 16-byte aligned"), (dict(A=A1 + 8), " A is not 16-byte aligned"), (dict(A=A0 + 64), " A overlaps S"),
]


@pytest.mark.parametrize("over,text", SYSTEM_REFUSALS, ids=[f"{i}" for i in range(len(SYSTEM_REFUSALS))])
def test_krr_system_refusals(over, text):
    rc, msg = _system(**over)
    assert rc == 1 and text.encode() in msg and b"clipfs_krr_system" in msg, msg


def _targets(labels=A0, labels_host=None, base_S=A1, ldbs=37, Et=A2, n=130, Cn=37, ldet=132, t=1.0):
    return _err(_lib.load().clipfs_krr_targets(labels, labels_host, base_S, ldbs, Et, n, Cn, ldet, t, None))


TARGETS_REFUSALS = [
    (dict(n=0), " n = "), (dict(Cn=0), " C = "), (dict(Cn=4097, ldbs=4097), " C = "), (dict(t=float("nan")), " t = "), (dict(t=float("inf")), " t = "),
    (dict(ldet=128), " ldet = "), (dict(ldet=134), " ldet = "), (dict(labels=None), " labels is NULL"), (dict(labels=A0 + 2), " labels is not 4-byte"),
    (dict(Et=None), " Et is NULL"), (dict(Et=A2 + 4), " Et is not 16-byte"), (dict(base_S=A1 + 2), " base_S is not 4-byte"),
    (dict(ldbs=36), " ldbs = "), (dict(Et=A1 + 16), " Et overlaps base_S"),
]


@pytest.mark.parametrize("over,text", TARGETS_REFUSALS, ids=[f"{i}" for i in range(len(TARGETS_REFUSALS))])
def test_krr_targets_refusals(over, text):
    rc, msg = _targets(**over)
    assert rc == 1 and text.encode() in msg and b"clipfs_krr_targets" in msg, msg


def test_labels_host_is_checked_before_anything_is_enqueued():
    good = (np.arange(130) % 37).astype(np.int32)
    for j, v in ((0, -1), (77, 37), (129, 1000)):
        host = good.copy()
        host[j] = v
        rc, msg = _targets(labels_host=host.ctypes.data)
        assert rc == 1 and f"labels_host[{j}] = {v}".encode() in msg, msg
        rc, msg = _fit(labels_host=host.ctypes.data)
        assert rc == 1 and f"labels_host[{j}] = {v}".encode() in msg and b"clipfs_krr_fit" in msg, msg


def _apply(X=A0, S=A1, At=A2, ldat=132, base=A3, ldbase=37, out=A4, ldo=37, B=70, n=130, Cn=37, d=64, beta=5.5):
    return _err(_lib.load().clipfs_krr_apply(X, S, At, ldat, base, ldbase, out, ldo, B, n, Cn, d, beta, None))


APPLY_REFUSALS = [
    (dict(d=6), " d = "), (dict(n=0), " n = "), (dict(Cn=4097, ldo=4097, ldbase=4097), " C = "), (dict(B=0), " B = "), (dict(beta=0.0), " beta = "),
    (dict(beta=101.0), " beta = "), (dict(ldat=128), " ldat = "), (dict(ldat=133), " ldat = "), (dict(ldo=36), " ldo = "),
    (dict(ldbase=30), " ldbase = "), (dict(X=None), " X is NULL"), (dict(S=None), " S is NULL"), (dict(At=None), " At is NULL"),
    (dict(out=None), " out is NULL"), (dict(X=A0 + 4), " X is not 16-byte"), (dict(At=A2 + 8), " At is not 16-byte"),
    (dict(out=A4 + 2), " out is not 4-byte"), (dict(base=A3 + 1), " base is not 4-byte"), (dict(out=A3 + 8), " out overlaps base"),
    (dict(out=A2 + 16), " out overlaps X, S or At"),
]


@pytest.mark.parametrize("over,text", APPLY_REFUSALS, ids=[f"{i}" for i in range(len(APPLY_REFUSALS))])
def test_krr_apply_refusals(over, text):
    rc, msg = _apply(**over)
    assert rc == 1 and text.encode() in msg and b"clipfs_krr_apply" in msg, msg


MEMBERS = ("shots", "labels", "A", "chol", "info", "Et", "At")


def _fit(params=None, labels_host=None, **over):
    p = _lib.new_krr_params(**{**dict(n=130, C=37, d=64, panel=256, beta=5.5, lambda_=1.0, t=1.0), **(params or {})})
    b = _lib.new_krr_buffers(base_S=9 << 32, ldbs=37, labels_host=labels_host)
    for k, name in enumerate(MEMBERS):
        setattr(b, name, (k + 1) << 32)
    for k, v in over.items():
        setattr(b, k, v)
    return _err(_lib.load().clipfs_krr_fit(C.byref(p), C.byref(b), None))


@pytest.mark.parametrize("params,name", [(dict(d=66), "d"), (dict(n=0), "n"), (dict(n=16385), "n"), (dict(C=0), "C"), (dict(panel=48), "panel"),
                                         (dict(beta=0.0), "beta"), (dict(beta=200.0), "beta"), (dict(lambda_=0.0), "lambda"),
                                         (dict(lambda_=float("nan")), "lambda"), (dict(t=float("inf")), "t")])
def test_krr_fit_refuses_bad_params(params, name):
    rc, msg = _fit(params)
    assert rc == 1 and f" {name} = ".encode() in msg, msg


@pytest.mark.parametrize("name", MEMBERS)
def test_krr_fit_refuses_a_null_or_misaligned_member(name):
    rc, msg = _fit(**{name: None})
    assert rc == 1 and f" {name} is NULL".encode() in msg and b"clipfs_krr_fit" in msg, msg
    rc, msg = _fit(**{name: ((MEMBERS.index(name) + 1) << 32) + 2})
    assert rc == 1 and f" {name} is not".encode() in msg and b"aligned" in msg, msg


def test_krr_fit_refuses_aliases_and_foreign_structs():
    lib = _lib.load()
    for name in ("A", "chol", "info", "Et", "At"):
        rc, msg = _fit(**{name: A0 + 16})  # inside shots
        assert rc == 1 and f" {name} aliases shots".encode() in msg, msg
    rc, msg = _fit(chol=(3 << 32) + 64)  # chol overlapping A other than as the same matrix
    assert rc == 1 and b" aliases " in msg, msg
    rc, msg = _fit(ldbs=36)
    assert rc == 1 and b" ldbs = " in msg
    p, b = _lib.new_krr_params(n=130, C=37, d=64, panel=256, beta=5.5, lambda_=1.0, t=1.0), _lib.new_krr_buffers()
    assert lib.clipfs_krr_fit(None, C.byref(b), None) == 1 and b"params" in lib.clipfs_last_error()
    assert lib.clipfs_krr_fit(C.byref(p), None, None) == 1 and b"buffers" in lib.clipfs_last_error()
    p.struct_size -= 4
    assert lib.clipfs_krr_fit(C.byref(p), C.byref(b), None) == 1 and b"params.struct_size" in lib.clipfs_last_error()
    p.struct_size += 4
    b.struct_size += 8
    assert lib.clipfs_krr_fit(C.byref(p), C.byref(b), None) == 1 and b"buffers.struct_size" in lib.clipfs_last_error()


def test_head_refuses_cpu_tensors_and_bad_input():
    import torch

    import proker
    f = torch.nn.functional.normalize(torch.randn(6, 8), dim=1)
    with pytest.raises(ValueError, match="no CPU path"):
        proker.ProKeRHead.from_features(f, torch.tensor([0, 0, 1, 1, 2, 2]), 3)
    for phrase in ("leave-one-out", "iterative refinement", "data parallelism", "fp16 storage", "16 384", "Nadaraya-Watson", "LOOP"):
        assert phrase in proker.__doc__ or phrase in proker.search_hp.__doc__, phrase
    head = proker.ProKeRHead(torch.zeros(6, 8), torch.zeros(3, 8), torch.zeros(1, dtype=torch.int32), beta=2.0, lam=0.5, target_scale=3.0,
                             panel=64)
    with pytest.raises(ValueError, match="no CPU path"):
        head(f)
    sd = head.state_dict()
    other = proker.ProKeRHead(torch.ones(6, 8), torch.ones(3, 8), torch.ones(1, dtype=torch.int32))
    other.load_state_dict(sd)
    assert (other.beta, other.lam, other.target_scale, other.panel) == (2.0, 0.5, 3.0, 64) and float(other.At.abs().sum()) == 0.0
    assert set(k for k in sd if not k.endswith("_extra_state")) == {"shots", "At", "info"}
