"""clipfs_augmix_plan / clipfs_augmix_batch without a GPU: every refusal returns CLIPFS_EINVAL and names its argument before
anything is enqueued (no device is opened: the fake, aligned addresses handed over are never dereferenced; the HOST tables
are real), nothing is written to the plan on refusal, and an accepted plan reports the buffer sizes and an LDS size that one
CU holds."""
import ctypes as C

import numpy as np
import pytest

from clipfs import _lib
from clipfs import augmix as A

POOL, SRC_DEV, RECS_DEV, OPS_DEV, COEF_DEV, DEPTH_DEV, W_DEV, M_DEV, MEAN, STD, BASE, CHAINS, OUT = (k << 36 for k in range(1, 14))
N, S, WIDTH = 3, 37, 2
H, Wd = 40, 57
POOL_BYTES = H * Wd * 3


def _tables():
    src = np.array([[0, H, Wd]], dtype=np.int64)
    recs = np.array([(0, 0, 0, H, Wd, v % 2, S, S, 0, 0, 0, 0) for v in range(N)], dtype=np.int32)
    r = A.sample_recipes(N, S, width=WIDTH, severity=3, seed=1)
    r.ops[0, 0, 0], r.ops[1, 0, 0], r.ops[2, 1, 0] = (A.POSTERIZE, 4), (A.SOLARIZE, 128), (A.AFFINE, 0)
    return dict(src=src, recs=recs, ops=r.ops, coef=r.coef, depth=r.depth, w=r.w, m=r.m)


def _call(tables=None, n=N, size=S, width=WIDTH, n_src=1, pool_bytes=POOL_BYTES, struct_size=None, recipe_null=False, **ptr):
    t = tables or _tables()
    p = dict(pool=POOL, src=t["src"].ctypes.data, src_dev=SRC_DEV, recs=t["recs"].ctypes.data, recs_dev=RECS_DEV,
             ops=t["ops"].ctypes.data, ops_dev=OPS_DEV, coef=t["coef"].ctypes.data, coef_dev=COEF_DEV,
             depth=t["depth"].ctypes.data, depth_dev=DEPTH_DEV, w=t["w"].ctypes.data, w_dev=W_DEV, m=t["m"].ctypes.data,
             m_dev=M_DEV, mean=MEAN, std=STD, base_u8=BASE, chains_u8=CHAINS, out=OUT)
    p.update(ptr)
    rc = _lib.AugmixRecipe()
    rc.struct_size = C.sizeof(_lib.AugmixRecipe) if struct_size is None else struct_size
    for name in ("ops", "coef", "depth", "w", "m"):
        setattr(rc, name, p[name])
        setattr(rc, name + "_dev", p[name + "_dev"])
    lib = _lib.load()
    code = lib.clipfs_augmix_batch(p["pool"], pool_bytes, p["src"], p["src_dev"], n_src, p["recs"], p["recs_dev"], n, size, width,
                                   None if recipe_null else C.byref(rc), p["mean"], p["std"], p["base_u8"], p["chains_u8"],
                                   p["out"], None)
    return code, lib.clipfs_last_error()


def test_bindings_and_header_agree():
    assert {"clipfs_augmix_plan", "clipfs_augmix_batch"} <= set(_lib.SIGNATURES)
    assert _lib.AUGMIX_CODES.index("affine") == A.AFFINE == 5 and _lib.AUGMIX_CODES.index("equalize") == A.EQUALIZE == 2


@pytest.mark.parametrize("n,size,width,name", [(0, 224, 3, "n"), (65537, 224, 3, "n"), (4, 7, 3, "S"), (4, 225, 3, "S"), (4, 336, 3, "S"),
                                               (4, 224, 0, "width"), (4, 224, 5, "width")])
def test_plan_refusals_write_nothing(n, size, width, name):
    lib = _lib.load()
    plan = _lib.AugmixPlan()
    plan.launches = -7
    assert lib.clipfs_augmix_plan(n, size, width, C.byref(plan)) == 1
    assert f" {name} = ".encode() in lib.clipfs_last_error(), lib.clipfs_last_error()
    assert plan.launches == -7 and plan.base_bytes == 0
    with pytest.raises(_lib.ClipfsError):
        _lib.augmix_plan(n, size, width)
    assert lib.clipfs_augmix_plan(4, 224, 3, None) == 1 and b"plan" in lib.clipfs_last_error()
    rc, msg = _call(n=n if name == "n" else N, size=size if name == "S" else S, width=width if name == "width" else WIDTH)
    assert rc == 1 and f" {name} = ".encode() in msg, msg


@pytest.mark.parametrize("n,size,width", [(1, 8, 1), (12, 37, 3), (512, 224, 3), (65536, 224, 4)])
def test_plan_of_an_accepted_call(n, size, width):
    p = _lib.augmix_plan(n, size, width)
    assert p["launches"] == 3 and set(p["launch"]) == {"base", "chains", "mix"}
    assert p["base_bytes"] == n * size * size * 3 and p["chains_bytes"] == n * width * size * size * 3
    assert p["out_floats"] == n * 3 * size * size
    assert p["launch"]["base"][:3] == (n, -(-size // 16), 256)
    assert p["launch"]["chains"][:3] == (n, width, 1024)
    assert p["launch"]["mix"] == (n, -(-size * size // 1024), 256, 0)
    assert size * size * 3 < p["lds_bytes"] == p["launch"]["chains"][3] <= 160 * 1024
    assert p["launch"]["base"][3] <= 160 * 1024


PTRS = ("pool", "src", "src_dev", "recs", "recs_dev", "ops", "ops_dev", "coef", "coef_dev", "depth", "depth_dev", "w", "w_dev",
        "m", "m_dev", "mean", "std", "base_u8", "chains_u8", "out")
ALIGN = dict(src_dev=8, recs_dev=4, ops_dev=4, coef_dev=8, depth_dev=4, w_dev=4, m_dev=4, mean=4, std=4, base_u8=16, chains_u8=16,
             out=16)


@pytest.mark.parametrize("name", PTRS)
def test_null_pointers(name):
    rc, msg = _call(**{name: None})
    assert rc == 1 and f" {name} is NULL".encode() in msg and b"clipfs_augmix_batch" in msg, msg


@pytest.mark.parametrize("name", sorted(ALIGN))
def test_misaligned_pointers(name):
    base = dict(src_dev=SRC_DEV, recs_dev=RECS_DEV, ops_dev=OPS_DEV, coef_dev=COEF_DEV, depth_dev=DEPTH_DEV, w_dev=W_DEV,
                m_dev=M_DEV, mean=MEAN, std=STD, base_u8=BASE, chains_u8=CHAINS, out=OUT)[name]
    rc, msg = _call(**{name: base + ALIGN[name] // 2})
    assert rc == 1 and f" {name} is not {ALIGN[name]}-byte aligned".encode() in msg, msg


def test_recipe_struct():
    rc, msg = _call(recipe_null=True)
    assert rc == 1 and b" recipe is NULL" in msg
    rc, msg = _call(struct_size=C.sizeof(_lib.AugmixRecipe) - 8)
    assert rc == 1 and b"recipe.struct_size" in msg


def _with(**edits):
    t = _tables()
    for name, (index, value) in edits.items():
        t[name][index] = value
    return t


RECIPE_REFUSALS = [
    (dict(ops=((0, 0, 0, 0), 6)), "ops[0, 0, 0] code = 6"), (dict(ops=((0, 0, 0, 0), -1)), "ops[0, 0, 0] code = -1"),
    (dict(ops=((0, 0, 0, 1), 0)), "ops[0, 0, 0] bits = 0"), (dict(ops=((0, 0, 0, 1), 9)), "ops[0, 0, 0] bits = 9"),
    (dict(ops=((1, 0, 0, 1), -1)), "ops[1, 0, 0] threshold = -1"), (dict(ops=((1, 0, 0, 1), 257)), "ops[1, 0, 0] threshold = 257"),
    (dict(depth=((2, 1), 4)), "depth[2, 1] = 4"), (dict(depth=((0, 0), -1)), "depth[0, 0] = -1"),
    (dict(coef=((2, 1, 0, 3), np.nan)), "coef[2, 1, 0, 3] is not finite"), (dict(coef=((2, 1, 0, 0), np.inf)), "coef[2, 1, 0, 0] is not finite"),
    (dict(w=((1, 1), np.nan)), "w[1, 1] is not finite"), (dict(w=((0, 0), -np.inf)), "w[0, 0] is not finite"),
    (dict(m=((2,), np.nan)), "m[2] is not finite"),
]


@pytest.mark.parametrize("edits,text", RECIPE_REFUSALS, ids=[t for _, t in RECIPE_REFUSALS])
def test_recipe_refusals(edits, text):
    rc, msg = _call(_with(**edits))
    assert rc == 1 and text.encode() in msg and b"clipfs_augmix_batch" in msg, msg


RECORD_REFUSALS = [
    (dict(recs=((1, 0), 1)), "view 1 names source 1 of 1"), (dict(recs=((1, 0), -1)), "view 1 names source -1"),
    (dict(recs=((0, 3), H + 1)), "view 0 box"), (dict(recs=((2, 1), -1)), "view 2 box"), (dict(recs=((0, 4), 0)), "view 0 box"),
    (dict(recs=((0, 5), 2)), "view 0 flip 2"), (dict(recs=((0, 10), 2)), "view 0 filter 2"),
    (dict(recs=((1, 6), S - 1)), "view 1 window"), (dict(recs=((1, 8), 1)), "view 1 window"), (dict(recs=((1, 9), -1)), "view 1 window"),
    (dict(src=((0, 1), 4097)), "source 0 is"), (dict(src=((0, 0), 3)), "source 0 lies outside"), (dict(src=((0, 0), -3)), "source 0 lies outside"),
]


@pytest.mark.parametrize("edits,text", RECORD_REFUSALS, ids=[f"{i}" for i in range(len(RECORD_REFUSALS))])
def test_everything_crop_batch_refuses_about_a_record(edits, text):
    rc, msg = _call(_with(**edits))
    assert rc == 1 and text.encode() in msg and b"clipfs_augmix_batch" in msg, msg


def test_too_many_taps_and_bad_counts():
    t = _tables()
    t["src"][0] = (0, 4096, 4096)
    t["recs"][0] = (0, 0, 0, 4096, 4096, 0, S, S, 0, 0, 1, 0)
    rc, msg = _call(t, pool_bytes=4096 * 4096 * 3)
    assert rc == 1 and b"view 0 needs" in msg and b"taps" in msg
    rc, msg = _call(n_src=0)
    assert rc == 1 and b" n_src = 0" in msg
    rc, msg = _call(pool_bytes=0)
    assert rc == 1 and b" pool_bytes = 0" in msg


BASE_BYTES, CHAINS_BYTES, OUT_BYTES = N * S * S * 3, N * WIDTH * S * S * 3, N * 3 * S * S * 4
OVERLAPS = [
    (dict(chains_u8=BASE), "chains_u8 overlaps base_u8"), (dict(chains_u8=BASE + 16 * ((BASE_BYTES - 1) // 16)), "chains_u8 overlaps base_u8"),
    (dict(base_u8=CHAINS + 16 * ((CHAINS_BYTES - 1) // 16)), "chains_u8 overlaps base_u8"),
    (dict(out=BASE + 16), "out overlaps base_u8"), (dict(base_u8=OUT + 16 * ((OUT_BYTES - 1) // 16)), "out overlaps base_u8"),
    (dict(out=CHAINS + 32), "out overlaps chains_u8"), (dict(chains_u8=OUT + 64), "out overlaps chains_u8"),
    (dict(base_u8=POOL + 16), "base_u8 overlaps pool"), (dict(chains_u8=POOL), "chains_u8 overlaps pool"),
    (dict(out=POOL + 16 * ((POOL_BYTES - 1) // 16)), "out overlaps pool"), (dict(pool=OUT + OUT_BYTES - 1), "out overlaps pool"),
]


@pytest.mark.parametrize("over,text", OVERLAPS, ids=[f"{i}" for i in range(len(OVERLAPS))])
def test_outputs_may_not_overlap(over, text):
    rc, msg = _call(**over)
    assert rc == 1 and text.encode() in msg, msg


def test_python_wrapper_refuses_bad_tables_before_touching_a_device():
    class FakePool:
        device = "cpu"
    r = A.sample_recipes(2, 37, width=2, seed=0)
    with pytest.raises(ValueError, match="records must be int32"):
        A.augmix_batch(FakePool(), np.zeros((2, 10), np.int32), r, 37)
    with pytest.raises(ValueError, match="the recipe is for 2 views"):
        A.augmix_batch(FakePool(), np.zeros((3, 12), np.int32), r, 37)
    with pytest.raises(ValueError, match="recipe.coef must be float64"):
        A.augmix_batch(FakePool(), np.zeros((2, 12), np.int32), r._replace(coef=r.coef.astype(np.float32)), 37)
