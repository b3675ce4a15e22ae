"""clipfs_tda_plan / clipfs_tda_adapt without a GPU: the plan's launch count does not depend on B or C, its LDS stays
within 160 KB, and every refusal of the header names its argument before anything is enqueued (no device is opened: the
pointers handed over are never dereferenced)."""
import ctypes as C

import pytest

from clipfs import _lib, ops


def _params(**over):
    return _lib.new_tda_params(**{**dict(C=37, d=132), **ops.TDA_DEFAULTS, **over})


def test_launch_count_is_independent_of_b_and_c():
    counts = {(B, Cn): ops.tda_plan(Cn, 512, B)["launches"] for B in (1, 256, 8192) for Cn in (5, 1000, 4096)}
    assert set(counts.values()) == {5}, counts
    assert ops.tda_plan(1000, 512, 256, update=False)["launches"] == 4
    assert ops.tda_plan(1000, 512, 256, pos_cap=0, neg_cap=0)["launches"] == 4  # no logits launch: out is z


@pytest.mark.parametrize("shape", [(1, 5, 64), (8192, 4096, 4096), (256, 1000, 512), (70, 5, 64)], ids=str)
def test_plan_lds_and_sizes(shape):
    B, Cn, d = shape
    p = ops.tda_plan(Cn, d, B)
    assert p["lds_bytes"] <= 160 * 1024 and p["lds_bytes"] == max(l[3] for l in p["launch"].values())
    assert sorted(p["launch"]) == sorted(_lib.TDA_LAUNCHES)
    assert p["launch"]["z"][:2] == ((Cn + 31) // 32, (B + 31) // 32)
    assert p["launch"]["logits"][:2] == ((B + 31) // 32, (Cn + p["class_chunk"] - 1) // p["class_chunk"])
    assert p["launch"]["scan"][0] * p["launch"]["scan"][2] >= Cn and p["launch"]["write"][0] == B
    assert (p["pos_entries"], p["neg_entries"]) == (Cn * 3 + B, Cn * 2 + B)
    assert (p["pos_key_floats"], p["neg_key_floats"], p["neg_mask_bytes"], p["mask_bytes"]) == (Cn * 3 * d, Cn * 2 * d,
                                                                                                  Cn * 2 * Cn, B * Cn)


PLAN_REFUSALS = [
    (dict(d=130), 8, "d"), (dict(d=0), 8, "d"), (dict(d=4100), 8, "d"),
    (dict(C=0), 8, "C"), (dict(C=4097), 8, "C"),
    (dict(), 0, "B"), (dict(), 8193, "B"),
    (dict(pos_cap=9), 8, "pos_cap"), (dict(neg_cap=-1), 8, "neg_cap"),
    (dict(pos_alpha=-1.0), 8, "pos_alpha"), (dict(pos_beta=float("nan")), 8, "pos_beta"),
    (dict(neg_alpha=float("inf")), 8, "neg_alpha"), (dict(neg_beta=-0.5), 8, "neg_beta"),
    (dict(logit_scale=float("inf")), 8, "logit_scale"),
]


@pytest.mark.parametrize("over,B,name", PLAN_REFUSALS, ids=[f"{n}-{i}" for i, (_, _, n) in enumerate(PLAN_REFUSALS)])
def test_plan_refusals_name_the_argument(over, B, name):
    lib = _lib.load()
    plan = _lib.TdaPlan()
    plan.launches = -7
    assert lib.clipfs_tda_plan(C.byref(_params(**over)), B, 1, C.byref(plan)) == 1
    assert name.encode() in lib.clipfs_last_error(), lib.clipfs_last_error()
    assert plan.launches == -7  # nothing written on refusal
    with pytest.raises(_lib.ClipfsError):
        _lib.tda_plan(_params(**over), B)


def test_plan_refuses_null_and_foreign_structs():
    lib = _lib.load()
    plan = _lib.TdaPlan()
    assert lib.clipfs_tda_plan(None, 8, 1, C.byref(plan)) == 1 and b"params" in lib.clipfs_last_error()
    assert lib.clipfs_tda_plan(C.byref(_params()), 8, 1, None) == 1 and b"plan" in lib.clipfs_last_error()
    p = _params()
    p.struct_size -= 4
    assert lib.clipfs_tda_plan(C.byref(p), 8, 1, C.byref(plan)) == 1 and b"struct_size" in lib.clipfs_last_error()


def _adapt_args(B=8):
    """Well-formed arguments made of fake, aligned, disjoint addresses (never dereferenced: every call below is refused)."""
    st, rec = _lib.TdaState(), _lib.TdaRecord()
    st.struct_size, rec.struct_size = C.sizeof(_lib.TdaState), C.sizeof(_lib.TdaRecord)
    addr = 1 << 30
    for name in _lib.TDA_STATE_FIELDS:
        setattr(st, name, addr)
        addr += 1 << 24
    for name in _lib.TDA_RECORD_FIELDS:
        setattr(rec, name, addr)
        addr += 1 << 24
    return dict(params=_params(), feats=addr, text=addr + (1 << 24), state=st, out=addr + (2 << 24), ldout=37, record=rec,
                B=B, update=1)


def _call(a):
    lib = _lib.load()
    rc = lib.clipfs_tda_adapt(C.byref(a["params"]) if a["params"] is not None else None, a["feats"], a["text"],
                              C.byref(a["state"]) if a["state"] is not None else None, a["out"], a["ldout"],
                              C.byref(a["record"]) if a["record"] is not None else None, a["B"], a["update"], None)
    return rc, lib.clipfs_last_error()


def _state_without(name):
    a = _adapt_args()
    setattr(a["state"], name, None)
    return a["state"]


def _record_without(name):
    a = _adapt_args()
    setattr(a["record"], name, None)
    return a["record"]


def _bad_size(s):
    s.struct_size += 8
    return s


ADAPT_REFUSALS = [
    ("feats", lambda a: None, "feats"), ("feats", lambda a: a["feats"] + 4, "feats"),
    ("text", lambda a: None, "text"), ("text", lambda a: a["text"] + 8, "text"),
    ("out", lambda a: None, "out"), ("out", lambda a: a["out"] + 4, "out"),
    ("ldout", lambda a: 36, "ldout"),
    ("out", lambda a: a["feats"], "out aliases"), ("out", lambda a: a["text"], "out aliases"),
    ("out", lambda a: a["state"].pos_keys, "out aliases"), ("out", lambda a: a["state"].neg_keys + 64, "out aliases"),
    ("state", lambda a: None, "state"), ("state", lambda a: _bad_size(a["state"]), "state.struct_size"),
    ("state", lambda a: _state_without("pos_keys"), "pos_keys"), ("state", lambda a: _state_without("neg_mask"), "neg_mask"),
    ("state", lambda a: _state_without("counter"), "counter"),
    ("record", lambda a: None, "record"), ("record", lambda a: _bad_size(a["record"]), "record.struct_size"),
    ("record", lambda a: _record_without("pos_evict"), "record"),
    ("B", lambda a: 8193, "B"), ("B", lambda a: 0, "B"),
    ("params", lambda a: None, "params"), ("params", lambda a: _params(d=6), "d"),
    ("params", lambda a: _params(pos_cap=9), "pos_cap"), ("params", lambda a: _params(neg_alpha=-1.0), "neg_alpha"),
]


@pytest.mark.parametrize("field,make,name", ADAPT_REFUSALS, ids=[f"{f}-{i}" for i, (f, _, _) in enumerate(ADAPT_REFUSALS)])
def test_adapt_refusals_name_the_argument(field, make, name):
    a = _adapt_args()
    a[field] = make(a)
    rc, msg = _call(a)
    assert rc == 1 and name.encode() in msg, msg
