"""clipfs_spd_* and clipfs_gda_* without a GPU: every refusal names its argument before anything is enqueued (no device is
opened: the fake, aligned addresses handed over are never dereferenced) and nothing is written on refusal."""
import ctypes as C

import numpy as np
import pytest

from clipfs import _lib, ops

A0, A1, A2, A3 = 1 << 32, 2 << 32, 3 << 32, 4 << 32  # fake, aligned, far apart


def _err(rc):
    lib = _lib.load()
    return rc, lib.clipfs_last_error()


# ---------------------------------------------------------------------------------------------------------------- SPD
@pytest.mark.parametrize("n,nrhs,name", [(0, 1, "n"), (6, 1, "n"), (1028, 1, "n"), (-4, 1, "n"), (64, 0, "nrhs"),
                                         (64, 65537, "nrhs")])
def test_spd_plan_refusals(n, nrhs, name):
    lib = _lib.load()
    plan = _lib.SpdPlan()
    plan.block = -7
    rc, msg = _err(lib.clipfs_spd_plan(n, nrhs, C.byref(plan)))
    assert rc == 1 and f" {name} = ".encode() in msg, msg
    assert plan.block == -7  # nothing written on refusal
    with pytest.raises(_lib.ClipfsError):
        ops.spd_plan(n, nrhs)
    rc, msg = _err(lib.clipfs_spd_plan(64, 1, None))
    assert rc == 1 and b"plan" in msg


def _factor(A=A0, lda=64, L=A1, ldl=64, n=64, info=A2):
    return _err(_lib.load().clipfs_spd_factor(A, lda, L, ldl, n, info, None))


FACTOR_REFUSALS = [
    (dict(n=6), " n = "), (dict(n=1028), " n = "), (dict(A=None), " A is NULL"), (dict(L=None), " L is NULL"),
    (dict(info=None), " info is NULL"), (dict(A=A0 + 4), " A is not 16-byte aligned"), (dict(L=A1 + 8), " L is not 16-byte aligned"),
    (dict(info=A2 + 2), " info is not 4-byte aligned"), (dict(lda=60), " lda = "), (dict(lda=66), " lda = "), (dict(ldl=32), " ldl = "),
    (dict(ldl=70), " ldl = "), (dict(L=A0, ldl=72, lda=64), " L overlaps A"), (dict(L=A0 + 64), " L overlaps A"),
    (dict(info=A0 + 16), " info overlaps"), (dict(info=A1 + 4 * (63 * 64 + 63)), " info overlaps"),
]


@pytest.mark.parametrize("over,text", FACTOR_REFUSALS, ids=[f"{i}" for i in range(len(FACTOR_REFUSALS))])
def test_spd_factor_refusals(over, text):
    rc, msg = _factor(**over)
    assert rc == 1 and text.encode() in msg and b"clipfs_spd_factor" in msg, msg


def _solve(L=A0, ldl=64, n=64, R=A1, ldr=64, X=A2, ldx=64, nrhs=70, alpha=1.0):
    return _err(_lib.load().clipfs_spd_solve(L, ldl, n, R, ldr, X, ldx, nrhs, alpha, None))


SOLVE_REFUSALS = [
    (dict(n=2), " n = "), (dict(nrhs=0), " nrhs = "), (dict(nrhs=65537), " nrhs = "), (dict(L=None), " L is NULL"),
    (dict(R=None), " R is NULL"), (dict(X=None), " X is NULL"), (dict(R=A1 + 4), " R is not 16-byte aligned"),
    (dict(X=A2 + 4), " X is not 16-byte aligned"), (dict(ldr=62), " ldr = "), (dict(ldx=60), " ldx = "), (dict(ldl=63), " ldl = "),
    (dict(alpha=float("nan")), " alpha = "), (dict(alpha=float("inf")), " alpha = "), (dict(X=A1, ldx=128), " X overlaps R"),
    (dict(X=A1 + 256), " X overlaps R"), (dict(X=A0 + 16), " X overlaps L"),
]


@pytest.mark.parametrize("over,text", SOLVE_REFUSALS, ids=[f"{i}" for i in range(len(SOLVE_REFUSALS))])
def test_spd_solve_refusals(over, text):
    rc, msg = _solve(**over)
    assert rc == 1 and text.encode() in msg and b"clipfs_spd_solve" in msg, msg


# ---------------------------------------------------------------------------------------------------------------- GDA
def _params(**over):
    return _lib.new_gda_params(**{**dict(M=112, C=37, d=132, prior=0, shrink=1.0), **over})


PLAN_REFUSALS = [
    (dict(d=130), "d"), (dict(d=0), "d"), (dict(d=1028), "d"), (dict(C=0), "C"), (dict(C=4097), "C"), (dict(M=1, C=1), "M"),
    (dict(M=65537), "M"), (dict(M=36), "M"), (dict(prior=2), "prior"), (dict(prior=-1), "prior"), (dict(shrink=-0.5), "shrink"),
    (dict(shrink=float("nan")), "shrink"), (dict(shrink=float("inf")), "shrink"),
]


@pytest.mark.parametrize("over,name", PLAN_REFUSALS, ids=[f"{n}-{i}" for i, (_, n) in enumerate(PLAN_REFUSALS)])
def test_gda_plan_refusals_name_the_argument(over, name):
    lib = _lib.load()
    plan = _lib.GdaPlan()
    plan.launches = -7
    rc, msg = _err(lib.clipfs_gda_plan(C.byref(_params(**over)), C.byref(plan)))
    assert rc == 1 and f" {name} = ".encode() in msg, msg
    assert plan.launches == -7
    with pytest.raises(_lib.ClipfsError):
        _lib.gda_plan(_params(**over))


def test_gda_plan_refuses_null_and_foreign_structs():
    lib = _lib.load()
    plan = _lib.GdaPlan()
    assert lib.clipfs_gda_plan(None, C.byref(plan)) == 1 and b"params" in lib.clipfs_last_error()
    assert lib.clipfs_gda_plan(C.byref(_params()), None) == 1 and b"plan" in lib.clipfs_last_error()
    p = _params()
    p.struct_size -= 4
    assert lib.clipfs_gda_plan(C.byref(p), C.byref(plan)) == 1 and b"struct_size" in lib.clipfs_last_error()
    with pytest.raises(ValueError, match="prior"):
        ops.gda_plan(112, 37, 132, prior="flat")


MEMBERS = [n for n in _lib.GDA_BUFFER_FIELDS if n != "offsets_host"]
WRITTEN = [n for n in MEMBERS if n not in ("shots", "offsets")]


def _fit_args(**over):
    b = _lib.new_gda_buffers()
    addr = 1 << 32
    for name in MEMBERS:
        setattr(b, name, addr)
        addr += 1 << 28
    return dict(params=_params(**over), buffers=b)


def _call(fn, a):
    lib = _lib.load()
    rc = getattr(lib, fn)(C.byref(a["params"]) if a["params"] is not None else None,
                          C.byref(a["buffers"]) if a["buffers"] is not None else None, None)
    return rc, lib.clipfs_last_error()


@pytest.mark.parametrize("name", MEMBERS)
def test_fit_refuses_a_null_or_misaligned_member(name):
    a = _fit_args()
    setattr(a["buffers"], name, None)
    rc, msg = _call("clipfs_gda_fit", a)
    assert rc == 1 and f"clipfs_gda_fit: {name} is NULL".encode() in msg, msg
    a = _fit_args()
    setattr(a["buffers"], name, getattr(a["buffers"], name) + 2)
    rc, msg = _call("clipfs_gda_fit", a)
    assert rc == 1 and f" {name} is not".encode() in msg and b"aligned" in msg, msg


@pytest.mark.parametrize("name", WRITTEN)
def test_fit_refuses_a_written_member_that_aliases_another(name):
    a = _fit_args()
    setattr(a["buffers"], name, a["buffers"].shots + 16)
    rc, msg = _call("clipfs_gda_fit", a)
    assert rc == 1 and f" {name} aliases shots".encode() in msg, msg


def _offsets(counts):
    o = np.zeros(len(counts) + 1, dtype=np.int32)
    o[1:] = np.cumsum(counts)
    return o


@pytest.mark.parametrize("fn", ["clipfs_gda_fit", "clipfs_gda_stats", "clipfs_gda_bias"])
def test_offsets_host_is_checked_before_anything_is_enqueued(fn):
    counts = np.full(37, 3)
    counts[0] = 4  # M = 112
    good = _offsets(counts)
    assert good[-1] == 112
    cases = []
    empty = counts.copy()
    empty[[11, 20]] = 0
    empty[0] += 6
    cases.append((_offsets(empty), b"class 11 owns no shot"))
    shifted = good.copy()
    shifted[0] = 1
    cases.append((shifted, b"offsets[0]"))
    down = good.copy()
    down[5] = down[4] - 1
    cases.append((down, b"offsets[5]"))
    short = good.copy()
    short[-1] = 111
    cases.append((short, b"offsets[C]"))
    for host, text in cases:
        a = _fit_args()
        a["buffers"].offsets_host = host.ctypes.data
        rc, msg = _call(fn, a)
        assert rc == 1 and text in msg and fn.encode() in msg, msg


STAGES = {"stats": ("shots", "offsets", "mu", "xt"), "shrink": ("gram", "tau"), "bias": ("offsets", "mu", "W", "b")}


@pytest.mark.parametrize("stage", sorted(STAGES))
def test_stage_refusals_name_the_member(stage):
    fn = f"clipfs_gda_{stage}"
    for name in STAGES[stage]:
        a = _fit_args()
        setattr(a["buffers"], name, None)
        rc, msg = _call(fn, a)
        assert rc == 1 and f"{fn}: {name} is NULL".encode() in msg, msg
    a = _fit_args()
    a["params"] = None
    assert _call(fn, a)[0] == 1 and b"params" in _lib.load().clipfs_last_error()
    a = _fit_args()
    a["buffers"] = None
    assert _call(fn, a)[0] == 1 and b"buffers" in _lib.load().clipfs_last_error()
    a = _fit_args()
    a["buffers"].struct_size += 8
    rc, msg = _call(fn, a)
    assert rc == 1 and b"buffers.struct_size" in msg
    rc, msg = _call(fn, _fit_args(d=130))
    assert rc == 1 and b" d = " in msg


def _search(g=A0, base=A1, ldbase=37, target=A2, alphas=A3, hits=A3 + (1 << 20), B=40, Cn=37, nA=9):
    return _err(_lib.load().clipfs_gda_search(g, base, ldbase, target, alphas, hits, B, Cn, nA, None))


SEARCH_REFUSALS = [
    (dict(B=0), " B = "), (dict(Cn=0), " C = "), (dict(Cn=4097), " C = "), (dict(nA=0), " nA = "), (dict(nA=1025), " nA = "),
    (dict(g=None), " g is NULL"), (dict(target=None), " target is NULL"), (dict(alphas=None), " alphas is NULL"),
    (dict(hits=None), " hits is NULL"), (dict(ldbase=36), " ldbase = "), (dict(g=A0 + 2), "aligned"), (dict(target=A2 + 4), "aligned"),
]


@pytest.mark.parametrize("over,text", SEARCH_REFUSALS, ids=[f"{i}" for i in range(len(SEARCH_REFUSALS))])
def test_search_refusals(over, text):
    rc, msg = _search(**over)
    assert rc == 1 and text.encode() in msg and b"clipfs_gda_search" in msg, msg


def test_head_refuses_cpu_tensors_and_bad_input():
    import torch

    import gda
    f = torch.nn.functional.normalize(torch.randn(6, 8), dim=1)
    with pytest.raises(ValueError, match="no CPU path"):
        gda.GDAHead.from_features(f, torch.tensor([0, 0, 1, 1, 2, 2]), 3)
    assert "classes without shots" in gda.__doc__ and "fp16 storage" in gda.__doc__ and "per-class covariances" in gda.__doc__
    head = gda.GDAHead(torch.zeros(3, 8), torch.zeros(3), torch.zeros(3, 8), torch.zeros(4, dtype=torch.int32),
                       torch.zeros(1, dtype=torch.int32), alpha=0.5, prior="empirical", shrink=2.0)
    with pytest.raises(ValueError, match="no CPU path"):
        head(f)
    sd = head.state_dict()
    other = gda.GDAHead(torch.ones(3, 8), torch.ones(3), torch.ones(3, 8), torch.ones(4, dtype=torch.int32),
                        torch.ones(1, dtype=torch.int32))
    other.load_state_dict(sd)
    assert (other.alpha, other.prior, other.shrink) == (0.5, "empirical", 2.0) and float(other.W.abs().sum()) == 0.0
    assert set(k for k in sd if not k.endswith("_extra_state")) == {"W", "b", "mu", "offsets", "info"}
