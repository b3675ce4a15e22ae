"""Every refusal of the OT matching entry points (include/clipfs.h "OT matching") by name, without a GPU: a refused call
returns CLIPFS_EINVAL before anything is enqueued, so the arguments here are host addresses that nothing dereferences.
No call in this file passes the checks."""
import ctypes as C

import pytest

B, M, CN, N, D = 2, 5, 3, 4, 8  # a valid shape: B, M, C, N, d
EPS, ITERS, SCALE = 0.1, 100, 100.0


@pytest.fixture(scope="module")
def lib():
    from clipfs import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def mem():
    """Named 64-byte-aligned host regions of one size, large enough for every argument at the valid shape."""
    sizes = dict(X=B * M * D, P=CN * N * D, mu=B * M, nu=CN * N, logits=B * CN, u=B * CN * M, v=B * CN * N, dlogits=B * CN,
                 dP=CN * N * D, dX=B * M * D)
    slot = (4 * max(sizes.values()) + 63) // 64 * 64
    raw = C.create_string_buffer(64 + slot * len(sizes))
    at = (C.addressof(raw) + 63) // 64 * 64
    out = {"_raw": raw}
    for i, k in enumerate(sizes):
        out[k] = at + i * slot
    return out


def _err(lib):
    return lib.clipfs_last_error().decode()


def _logits(lib, mem, B=B, M=M, Cn=CN, N=N, d=D, eps=EPS, iters=ITERS, scale=SCALE, ldl=None, **ptr):
    a = {k: ptr.get(k, mem[k]) for k in ("X", "P", "mu", "nu", "logits", "u", "v")}
    return lib.clipfs_ot_logits(a["X"], a["P"], a["mu"], a["nu"], a["logits"], Cn if ldl is None else ldl, a["u"], a["v"], B, M,
                                Cn, N, d, eps, iters, scale, None)


def _bwd(lib, mem, B=B, M=M, Cn=CN, N=N, d=D, eps=EPS, scale=SCALE, ldd=None, accumulate=0, **ptr):
    a = {k: ptr.get(k, mem[k]) for k in ("X", "P", "u", "v", "dlogits", "dP", "dX")}
    return lib.clipfs_ot_bwd(a["X"], a["P"], a["u"], a["v"], a["dlogits"], Cn if ldd is None else ldd, a["dP"], a["dX"], B, M, Cn,
                             N, d, eps, scale, accumulate, None)


SHAPES = [(dict(d=6), "d = 6"), (dict(d=1028), "d = 1028"), (dict(d=0), "d = 0"), (dict(M=0), "M = 0"), (dict(M=257), "M = 257"),
          (dict(N=0), "N = 0"), (dict(N=33), "N = 33"), (dict(B=0), "B = 0"), (dict(Cn=0), "C = 0"),
          (dict(B=(1 << 20) + 1), "B = 1048577"), (dict(Cn=(1 << 20) + 1), "C = 1048577"),
          (dict(B=1 << 17, M=256), "B M"), (dict(Cn=1 << 20, N=32), "C N"), (dict(B=1 << 15, Cn=1 << 14), "B C")]


@pytest.mark.parametrize("kw,name", SHAPES, ids=[n for _, n in SHAPES])
def test_shape_refusals(lib, mem, kw, name):
    from clipfs import _lib, ops
    s = dict(B=B, M=M, Cn=CN, N=N, d=D)
    s.update(kw)
    plan = _lib.OtPlan()
    plan.threads = 77
    assert lib.clipfs_ot_plan(s["B"], s["M"], s["Cn"], s["N"], s["d"], C.byref(plan)) == 1
    assert name in _err(lib) and "clipfs_ot_plan" in _err(lib)
    assert plan.threads == 77  # nothing written on refusal
    assert _logits(lib, mem, **kw) == 1 and name in _err(lib) and "clipfs_ot_logits" in _err(lib)
    assert _bwd(lib, mem, **kw) == 1 and name in _err(lib) and "clipfs_ot_bwd" in _err(lib)
    with pytest.raises(_lib.ClipfsError, match=name):
        ops.ot_plan(s["B"], s["M"], s["Cn"], s["N"], s["d"])


def test_plan_null(lib):
    assert lib.clipfs_ot_plan(B, M, CN, N, D, None) == 1 and "plan is NULL" in _err(lib)


@pytest.mark.parametrize("eps", (0.04, 11.0, float("nan")))
def test_eps_refusals(lib, mem, eps):
    assert _logits(lib, mem, eps=eps) == 1 and "eps = " in _err(lib) and "[0.05, 10]" in _err(lib)
    assert _bwd(lib, mem, eps=eps) == 1 and "eps = " in _err(lib)


@pytest.mark.parametrize("iters", (0, 1001, -1))
def test_iters_refusals(lib, mem, iters):
    assert _logits(lib, mem, iters=iters) == 1 and f"iters = {iters}" in _err(lib)


@pytest.mark.parametrize("scale", (float("inf"), float("nan")))
def test_scale_refusals(lib, mem, scale):
    assert _logits(lib, mem, scale=scale) == 1 and "scale" in _err(lib)
    assert _bwd(lib, mem, scale=scale) == 1 and "scale" in _err(lib)


def test_leading_dimension_refusals(lib, mem):
    assert _logits(lib, mem, ldl=CN - 1) == 1 and "ldl = 2" in _err(lib)
    assert _bwd(lib, mem, ldd=CN - 1) == 1 and "ldd = 2" in _err(lib)


@pytest.mark.parametrize("name", ("X", "P", "logits", "u", "v"))
def test_logits_null_pointers(lib, mem, name):
    assert _logits(lib, mem, **{name: None}) == 1 and f"{name} is NULL" in _err(lib)


@pytest.mark.parametrize("name", ("X", "P", "u", "v", "dlogits", "dP"))
def test_bwd_null_pointers(lib, mem, name):
    assert _bwd(lib, mem, **{name: None}) == 1 and f"{name} is NULL" in _err(lib)


@pytest.mark.parametrize("name,align,off", (("X", 16, 4), ("P", 16, 8), ("mu", 4, 2), ("nu", 4, 1), ("logits", 4, 2), ("u", 4, 1),
                                            ("v", 4, 3)))
def test_logits_misaligned(lib, mem, name, align, off):
    assert _logits(lib, mem, **{name: mem[name] + off}) == 1 and f"{name} is not {align}-byte aligned" in _err(lib)


@pytest.mark.parametrize("name,align,off", (("X", 16, 4), ("P", 16, 12), ("u", 4, 2), ("v", 4, 2), ("dlogits", 4, 1), ("dP", 16, 4),
                                            ("dX", 16, 8)))
def test_bwd_misaligned(lib, mem, name, align, off):
    assert _bwd(lib, mem, **{name: mem[name] + off}) == 1 and f"{name} is not {align}-byte aligned" in _err(lib)


@pytest.mark.parametrize("out,inp", (("logits", "X"), ("logits", "P"), ("u", "X"), ("v", "P"), ("u", "mu"), ("v", "nu"),
                                     ("logits", "u"), ("u", "v")))
def test_logits_outputs_overlapping(lib, mem, out, inp):
    assert _logits(lib, mem, **{out: mem[inp]}) == 1 and "overlaps" in _err(lib) and out in _err(lib) and inp in _err(lib)
    # a partial overlap: the output begins 16 bytes into the other region
    assert _logits(lib, mem, **{out: mem[inp] + 16}) == 1 and "overlaps" in _err(lib)


@pytest.mark.parametrize("out,inp", (("dP", "P"), ("dP", "X"), ("dX", "X"), ("dX", "P"), ("dP", "u"), ("dX", "v"), ("dP", "dlogits"),
                                     ("dX", "dP")))
def test_bwd_outputs_overlapping(lib, mem, out, inp):
    assert _bwd(lib, mem, **{out: mem[inp]}) == 1 and "overlaps" in _err(lib) and out in _err(lib) and inp in _err(lib)
