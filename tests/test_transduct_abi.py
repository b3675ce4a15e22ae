"""clipfs_transduct_plan and the transductive entry points without a GPU: the launch count of a fit is a closed form of
(outer, inner, chunks), the LDS stays within 160 KB, the kNN workspace is O(N k chunks) (the N x N similarities are never
stored), and every refusal names its argument before anything is enqueued (no device is opened: the addresses handed
over are never dereferenced)."""
import ctypes as C

import numpy as np
import pytest

from clipfs import _lib, ops


def _params(**over):
    return _lib.new_transduct_params(**{**dict(N=150, C=37, d=132, M=0, knn_chunks=0), **ops.TRANSDUCT_DEFAULTS, **over})


@pytest.mark.parametrize("chunks", [1, 2, 5])
def test_launch_count_is_a_closed_form(chunks):
    for outer, inner in ((10, 5), (1, 1), (3, 7)):
        counts = {(N, Cn): ops.transduct_plan(N, Cn, 512, knn_chunks=chunks, outer=outer, inner=inner)["launches"]
                  for N in (70, 8192, 131072) for Cn in (5, 1000, 4096)}
        assert set(counts.values()) == {6 + (chunks > 1) + outer * (inner + 4)}, counts
    assert ops.transduct_plan(8192, 1000, 512, M=16000, knn_chunks=chunks)["launches"] == 6 + (chunks > 1) + 10 * 9


def test_the_plan_chooses_chunks_only_where_row_tiles_are_few():
    assert ops.transduct_plan(50000, 1000, 512)["knn_chunks"] == 1
    p = ops.transduct_plan(2048, 1000, 512)
    assert 1 < p["knn_chunks"] <= 64 and p["launch"]["knn"][:2] == (64, p["knn_chunks"]) and "knn_merge" in p["launch"]
    assert ops.transduct_plan(70, 5, 64)["knn_chunks"] == 3  # never more chunks than key tiles
    assert "knn_merge" not in ops.transduct_plan(70, 5, 64, knn_chunks=1)["launch"]


@pytest.mark.parametrize("shape", [(70, 5, 64), (150, 37, 132), (8192, 1000, 512), (131072, 4096, 4096), (50000, 1000, 512)],
                         ids=str)
@pytest.mark.parametrize("chunks", [0, 1, 5])
def test_plan_lds_grids_and_workspace(shape, chunks):
    N, Cn, d = shape
    p = ops.transduct_plan(N, Cn, d, knn_chunks=chunks)
    k = ops.TRANSDUCT_DEFAULTS["k"]
    assert p["lds_bytes"] <= 160 * 1024 and p["lds_bytes"] == max(l[4] for l in p["launch"].values())
    rt, ct = (N + 31) // 32, (Cn + 31) // 32
    assert p["launch"]["knn"][:2] == (rt, p["knn_chunks"])
    assert p["launch"]["logits"][:2] == p["launch"]["u"][:2] == (ct, rt)
    assert p["launch"]["z_step"][0] * 4 >= N and p["launch"]["init"][0] == ct and p["launch"]["shots"][0] == Cn
    assert p["class_chunk"] >= Cn
    # the affinity's workspace: the chunks' partial lists, nothing that grows like N^2.  The documented constant is 0.
    assert p["knn_work_bytes"] <= N * k * p["knn_chunks"] * 16
    assert p["knn_work_bytes"] == (p["knn_chunks"] * N * k * 8 if p["knn_chunks"] > 1 else 0)
    # the statistics' partial sums do not depend on N at all
    assert p["stat_splits"] <= 8 and p["stat_rows"] % 16 == 0 and p["stat_splits"] * p["stat_rows"] >= N
    assert p["stat_work_floats"] == p["stat_splits"] * Cn * (d + 1) and p["launch"]["stats"][2] == p["stat_splits"]
    assert p["nc_floats"] == N * Cn


PLAN_REFUSALS = [
    (dict(d=130), "d"), (dict(d=0), "d"), (dict(d=4100), "d"), (dict(C=0), "C"), (dict(C=4097), "C"),
    (dict(N=3, k=3), "N"), (dict(N=7), "N"), (dict(N=131073), "N"), (dict(k=0), "k"), (dict(k=9), "k"),
    (dict(init_top=0), "init_top"), (dict(init_top=17), "init_top"), (dict(M=-1), "M"), (dict(M=65537), "M"),
    (dict(outer=0), "outer"), (dict(inner=0), "inner"), (dict(knn_chunks=-1), "knn_chunks"), (dict(knn_chunks=65), "knn_chunks"),
    (dict(logit_scale=float("inf")), "logit_scale"), (dict(logit_scale=-1.0), "logit_scale"), (dict(lam=float("nan")), "lam"),
    (dict(lam=-0.5), "lam"), (dict(shot_weight=-1.0), "shot_weight"), (dict(n_min=float("nan")), "n_min"),
    (dict(var_floor=-1e-6), "var_floor"), (dict(var_floor=float("inf")), "var_floor"),
]


@pytest.mark.parametrize("over,name", PLAN_REFUSALS, ids=[f"{n}-{i}" for i, (_, n) in enumerate(PLAN_REFUSALS)])
def test_plan_refusals_name_the_argument(over, name):
    lib = _lib.load()
    plan = _lib.TransductPlan()
    plan.launches = -7
    assert lib.clipfs_transduct_plan(C.byref(_params(**over)), C.byref(plan)) == 1
    assert f" {name} ".encode() in lib.clipfs_last_error(), lib.clipfs_last_error()
    assert plan.launches == -7  # nothing written on refusal
    with pytest.raises(_lib.ClipfsError):
        _lib.transduct_plan(_params(**over))


def test_plan_refuses_null_and_foreign_structs():
    lib = _lib.load()
    plan = _lib.TransductPlan()
    assert lib.clipfs_transduct_plan(None, C.byref(plan)) == 1 and b"params" in lib.clipfs_last_error()
    assert lib.clipfs_transduct_plan(C.byref(_params()), None) == 1 and b"plan" in lib.clipfs_last_error()
    p = _params()
    p.struct_size -= 4
    assert lib.clipfs_transduct_plan(C.byref(p), C.byref(plan)) == 1 and b"struct_size" in lib.clipfs_last_error()


def _fit_args(M=74, **over):
    """Well-formed arguments made of fake, aligned, disjoint addresses (never dereferenced: every call below is refused)."""
    b = _lib.new_transduct_buffers()
    addr = 1 << 32
    for name in _lib.TRANSDUCT_BUFFER_FIELDS:
        if name != "shot_labels_host":
            setattr(b, name, addr)
            addr += 1 << 28
    return dict(params=_params(M=M, knn_chunks=2, **over), buffers=b)


def _fit(a):
    lib = _lib.load()
    rc = lib.clipfs_transduct_fit(C.byref(a["params"]) if a["params"] is not None else None,
                                  C.byref(a["buffers"]) if a["buffers"] is not None else None, None)
    return rc, lib.clipfs_last_error()


MEMBERS = [n for n in _lib.TRANSDUCT_BUFFER_FIELDS if n != "shot_labels_host"]
WRITTEN = [n for n in MEMBERS if n not in ("feats", "text", "shots", "shot_labels")]


@pytest.mark.parametrize("name", MEMBERS)
def test_fit_refuses_a_null_or_misaligned_member(name):
    a = _fit_args()
    setattr(a["buffers"], name, None)
    rc, msg = _fit(a)
    assert rc == 1 and f" {name} is NULL".encode() in msg, msg
    a = _fit_args()
    setattr(a["buffers"], name, getattr(a["buffers"], name) + 2)
    rc, msg = _fit(a)
    assert rc == 1 and f" {name} is not".encode() in msg and b"aligned" in msg, msg


@pytest.mark.parametrize("name", WRITTEN)
def test_fit_refuses_a_written_member_that_aliases_another(name):
    a = _fit_args()
    setattr(a["buffers"], name, a["buffers"].feats + 16)
    rc, msg = _fit(a)
    assert rc == 1 and f" {name} aliases feats".encode() in msg, msg


def test_fit_allows_null_shots_without_shots_and_null_work_with_one_chunk():
    # not refused for the members: the refusal that stops the call (and keeps the fake addresses unread) is the label check
    a = _fit_args(M=0)
    a["buffers"].shots = a["buffers"].shot_labels = None
    a["params"].knn_chunks = 1
    a["buffers"].knn_work = None
    a["params"].struct_size += 4
    rc, msg = _fit(a)
    assert rc == 1 and b"struct_size" in msg
    # with M = 0 and one chunk the planned sizes of those members are 0
    p = ops.transduct_plan(150, 37, 132, knn_chunks=1)
    assert p["knn_work_bytes"] == 0


def test_fit_refuses_labels_out_of_range_and_foreign_structs():
    for bad in (-1, 37):
        a = _fit_args()
        host = np.arange(74, dtype=np.int32) % 37
        host[50] = bad
        a["buffers"].shot_labels_host = host.ctypes.data
        rc, msg = _fit(a)
        assert rc == 1 and b"shot_labels[50]" in msg, msg
    a = _fit_args()
    a["buffers"].struct_size += 8
    rc, msg = _fit(a)
    assert rc == 1 and b"buffers.struct_size" in msg
    a = _fit_args()
    a["buffers"] = None
    rc, msg = _fit(a)
    assert rc == 1 and b"buffers" in msg
    a = _fit_args()
    a["params"] = None
    rc, msg = _fit(a)
    assert rc == 1 and b"params" in msg
    rc, msg = _fit(_fit_args(k=9))
    assert rc == 1 and b" k " in msg


STAGES = {
    "logy": ("feats", "text", "logy", "z", "zs_labels"),
    "knn": ("feats", "nbr", "w", "knn_work"),
    "init": ("feats", "shots", "shot_labels", "logy", "shot_n", "shot_G", "Q", "sel", "mu", "mup", "var"),
    "u": ("feats", "logy", "mu", "mup", "bias", "u"),
}


@pytest.mark.parametrize("stage", sorted(STAGES))
def test_stage_refusals_name_the_member(stage):
    lib = _lib.load()
    fn = getattr(lib, f"clipfs_transduct_{stage}")
    for name in STAGES[stage]:
        a = _fit_args()
        setattr(a["buffers"], name, None)
        assert fn(C.byref(a["params"]), C.byref(a["buffers"]), None) == 1
        assert f"clipfs_transduct_{stage}: {name} is NULL".encode() in lib.clipfs_last_error(), lib.clipfs_last_error()
    assert fn(None, C.byref(_fit_args()["buffers"]), None) == 1 and b"params" in lib.clipfs_last_error()
    assert fn(C.byref(_fit_args()["params"]), None, None) == 1 and b"buffers" in lib.clipfs_last_error()


def test_z_step_and_stats_refusals():
    lib = _lib.load()
    a = _fit_args()
    b, p = a["buffers"], a["params"]
    zi, zo = b.z, b.z2
    call = lambda zin, zout: (lib.clipfs_transduct_z_step(C.byref(p), C.byref(b), zin, zout, None, None), lib.clipfs_last_error())
    rc, msg = call(None, zo)
    assert rc == 1 and b"z_in" in msg
    rc, msg = call(zi, None)
    assert rc == 1 and b"z_out" in msg
    rc, msg = call(zi, zo + 4)
    assert rc == 1 and b"z_out" in msg and b"aligned" in msg
    for other in (zi, b.u, b.nbr, b.w):
        rc, msg = call(zi, other)
        assert rc == 1 and b"z_out aliases" in msg, msg
    b.nbr = None
    rc, msg = call(zi, zo)
    assert rc == 1 and b" nbr is NULL" in msg
    a = _fit_args()
    assert lib.clipfs_transduct_stats(C.byref(a["params"]), C.byref(a["buffers"]), None, None) == 1
    assert b"z_in" in lib.clipfs_last_error()
    a["buffers"].stat_work = None
    assert lib.clipfs_transduct_stats(C.byref(a["params"]), C.byref(a["buffers"]), a["buffers"].z, None) == 1
    assert b" stat_work is NULL" in lib.clipfs_last_error()


def test_ops_refuse_unknown_hyper_parameters():
    with pytest.raises(KeyError, match="alpha"):
        ops.transduct_plan(70, 5, 64, alpha=1.0)
    assert set(ops.TRANSDUCT_DEFAULTS) == {"logit_scale", "k", "init_top", "lam", "shot_weight", "outer", "inner", "n_min",
                                           "var_floor"}
