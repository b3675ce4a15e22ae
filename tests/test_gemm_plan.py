"""Host-only: clipfs_gemm_plan -- the function clipfs_gemm_nt executes for the exact fp32 and the 16-bit-plane kernels --
answers the full plan of every row of gemm_plan_cases.py, refuses what the entry point refuses with the same message, and
agrees with the five shape-only queries wherever the route can split.  A retune of the schedule fails here, loudly and
without a GPU.  The counterpart of test_gemm_f16_plan.py for csrc/gemm.hip."""
import ctypes as C
import json
import re
import subprocess

import pytest

import gemm_plan_cases as cases
from gemm_plan_cases import KERNELS, PLAN, PLAN_FIELDS, PLAN_TABLE, fake_pointers, gemm_args, query_plan

IN_PROCESS = [c for c in PLAN_TABLE if c.env is None]


@pytest.fixture(scope="module")
def lib():
    from clipfs import _lib
    return _lib.load()


@pytest.fixture(scope="module", autouse=True)
def no_aid_in_this_process():
    import os
    set_ = sorted(k for k in os.environ if k.startswith(cases.AID_PREFIXES))
    assert not set_, f"the table is stated for the default dispatch; unset {set_}"


@pytest.mark.parametrize("c", IN_PROCESS, ids=[c.name for c in IN_PROCESS])
def test_row_gets_its_plan(lib, c):
    assert query_plan(c) == c.plan


@pytest.mark.parametrize("aid", cases.aids())
def test_rows_under_a_cached_aid(aid):
    """The aids are read once per process: their rows are asked in one fresh child per aid."""
    r = subprocess.run(cases.child_command(f"cases.print_plans({aid!r})"), env=cases.child_env(aid), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("PLANS ")][-1]
    assert json.loads(line[6:]) == {c.name: c.plan for c in PLAN_TABLE if c.env == aid}


def test_table_covers_what_it_is_there_for():
    assert {c.plan["kernel"] for c in PLAN_TABLE} == set(KERNELS), "every kernel id"
    assert all(tuple(c.plan) == PLAN_FIELDS for c in PLAN_TABLE), "the full plan per row"
    assert all(0 < c.plan["lds_bytes"] <= 160 * 1024 for c in PLAN_TABLE), "a CU has 160 KiB of LDS"
    assert {c.env.split("=")[0] for c in PLAN_TABLE if c.env} == {
        "CLIPFS_GEMM_BM", "CLIPFS_GEMM_SPLITS", "CLIPFS_GEMM_GM", "CLIPFS_GEMM_LDS_PAD", "CLIPFS_GEMM_GLDS", "CLIPFS_BF16_TILE"}
    for c in cases.SCHEDULE_CLASSES:
        full, bare = PLAN[f"class_{c.name}"].plan, PLAN[f"class_{c.name}_bare"].plan
        assert bare["splits"] == 1 and bare["want_splits"] == full["want_splits"] == full["splits"]
    assert {c.scratch for c in PLAN_TABLE} == {"full", "none", "misaligned", "few_counters"}
    planes = [c for c in PLAN_TABLE if c.planes and not c.ldb_pad and c.env is None]
    assert {(c.plan["kernel"], c.plan["planes"]) for c in planes} == {(k, n) for k in ("planes64", "planes128") for n in (1, 2)}
    assert {(c.plan["planes"], c.plan["lds_bytes"]) for c in planes if c.plan["kernel"] == "planes64"} == {(2, 49152), (1, 24576)}


def test_kernel_ids_and_struct_match_the_header():
    import os
    from clipfs import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "clipfs.h")).read()
    ids = {name: int(v) for name, v in re.findall(r"#define CLIPFS_GEMM_([A-Z0-9_]+) (\d+)", header)}
    assert [k for k, _ in sorted(ids.items(), key=lambda kv: kv[1])] == [n.upper() for n in _lib.GEMM_KERNELS]
    assert sorted(ids.values()) == list(range(len(KERNELS))) and _lib.GEMM_KERNELS == KERNELS
    body = re.search(r"struct clipfs_gemm_plan \{(.*?)\};", re.sub(r"/\*.*?\*/", "", header, flags=re.S), flags=re.S).group(1)
    fields = [(t, n.strip()) for t, decl in re.findall(r"(int|size_t) ([^;]+);", body) for n in decl.split(",")]
    assert fields == [("size_t" if t is C.c_size_t else "int", n) for n, t in _lib.GemmPlan._fields_]
    assert tuple(n for _, n in fields) == PLAN_FIELDS
    assert "#define CLIPFS_ABI_VERSION 2" in header and _lib.load().clipfs_abi_version() == 2


def test_shape_only_queries_keep_their_answers_where_the_plan_differs(lib):
    """K % 32 != 0, patch mode and planes: the legacy queries describe a dense fp32 product with scratch"""
    assert lib.clipfs_gemm_tile_rows(50, 64) == 32 and PLAN["ktail_tiny"].plan["tile_rows"] == 64
    c = PLAN["patch32_vit_b32"]
    assert (c.M, c.N, c.K) == (98, 768, 3072)
    assert lib.clipfs_gemm_tile_rows(98, 768) == 32 and lib.clipfs_gemm_splits(98, 768, 3072) == 8
    assert lib.clipfs_gemm_workspace_floats(98, 768, 3072) == 8 * 24 * 32 * 128 and c.plan["workspace_floats"] == 0
    # K tail: a split and a workspace are reported, the product never splits
    assert lib.clipfs_gemm_splits(250, 403, 1060) == 8 and lib.clipfs_gemm_workspace_floats(250, 403, 1060) > 0
    g = gemm_args(250, 403, 1060)
    from clipfs import _lib
    p = _lib.gemm_plan(g)
    assert (p["kernel"], p["splits"], p["want_splits"], p["workspace_floats"], p["counter_ints"]) == ("generic", 1, 1, 0, 0)
    c = PLAN["bf16x3_per_rank_unsplit"]
    assert lib.clipfs_gemm_splits(c.M, c.N, c.K) == 3 and c.plan["want_splits"] == 1


def test_wrappers_equal_the_plan_over_a_sweep(lib):
    """Dense fp32 with all the scratch a call could want: the five shape-only queries are the plan's fields wherever the
    route can split (K % 32 == 0); the generic kernel reports 1 / 0 / 0."""
    g = gemm_args(1, 64, 96, scratch="none")
    g.workspace, g.counters = fake_pointers()["workspace"], fake_pointers()["counters"]
    g.workspace_floats = g.counters_ints = 1 << 40
    plan = __import__("clipfs._lib", fromlist=["GemmPlan"]).GemmPlan()
    n = 0
    for M in range(1, 20001, 97):
        for N in (64, 200, 512, 768, 1536, 2048, 3072):
            for K in (96, 100, 128, 512, 768, 3072):
                g.M, g.N, g.K, g.lda, g.ldb, g.ldc = M, N, K, K, K, N
                assert lib.clipfs_gemm_plan(C.byref(g), C.byref(plan)) == 0, lib.clipfs_last_error()
                got = (plan.want_splits, plan.splits, plan.workspace_floats, plan.counter_ints)
                if K % 32:
                    assert plan.kernel == KERNELS.index("generic") and plan.tile_rows == 64 and plan.mix_rows64 == 0
                    assert got == (1, 1, 0, 0), (M, N, K, got)
                else:
                    s = lib.clipfs_gemm_splits(M, N, K)
                    assert got == (s, s, lib.clipfs_gemm_workspace_floats(M, N, K), lib.clipfs_gemm_counter_ints(M, N, K)), (M, N, K, got)
                    assert plan.tile_rows == lib.clipfs_gemm_tile_rows(M, N), (M, N, K)
                    assert plan.mix_rows64 == lib.clipfs_gemm_mixed_rows64(M, N, K), (M, N, K)
                    assert (plan.kernel == KERNELS.index("mixed")) == (plan.mix_rows64 > 0)
                    tiles = cases.ceil_div(M, plan.tile_rows) * cases.ceil_div(N, 128)
                    if not plan.mix_rows64:
                        assert plan.grid == tiles * plan.splits and (plan.counter_ints == tiles or s == 1)
                assert 0 < plan.lds_bytes <= 160 * 1024 and plan.block == 256 and plan.grid > 0
                n += 1
    assert n == 207 * 7 * 6


# ------------------------------------------------------------------ refusals
def _good(**kw):
    return gemm_args(18 if "patch" in kw else 1600, 768, 768, **kw)


def _set(**fields):
    def change(g):
        for k, v in fields.items():
            setattr(g, k, v)
    return change


PATCH16 = dict(patch=(2, 48, 16))   # 18 x N x 768
REFUSALS = [
    ("stale_header", {}, lambda g: setattr(g, "struct_size", g.struct_size - 8), b"struct_size"),
    ("bad_dims", {}, _set(M=0), b"bad dims 0 768 768"),
    ("a_f16", {}, _set(A_f16=0x1000), b"clipfs_gemm_f16_plan"),
    ("c_f16", {}, _set(C_f16=0x1000), b"C_f16 / aux_f16 belong to the f16 x f16 kernel only"),
    ("aux_f16", {}, _set(aux_f16=1), b"C_f16 / aux_f16 belong to the f16 x f16 kernel only"),
    ("null_a", {}, _set(A=0), b"null operand"),
    ("null_c", {}, _set(C=0), b"null operand"),
    ("k_not_x4", {}, _set(K=766), b"K and ldb must be multiples of 4, B 16-byte aligned"),
    ("b_misaligned", {}, lambda g: setattr(g, "B", g.B + 4), b"K and ldb must be multiples of 4, B 16-byte aligned"),
    ("ldb_small", {}, _set(ldb=764), b"leading dimension too small"),
    ("ldc_small", {}, _set(ldc=767), b"leading dimension too small"),
    ("bad_act", {}, _set(act=4), b"bad act 4"),
    ("relu_with_planes", dict(planes="bf16x3"), _set(act=3), b"act 3 (ReLU) belongs to the exact fp32 kernels"),
    ("act2_without_aux_in", {}, _set(act=2), b"act 2 needs aux_in"),
    ("ldres_small", {}, _set(residual=0x2000, ldres=767), b"ldres too small"),
    ("lda_small", {}, _set(lda=764), b"lda must be a multiple of 4 and >= K, A 16-byte aligned"),
    ("a_misaligned", {}, lambda g: setattr(g, "A", g.A + 4), b"lda must be a multiple of 4 and >= K, A 16-byte aligned"),
    ("bad_a_mode", {}, _set(a_mode=2), b"bad a_mode 2"),
    ("patch_not_dividing", PATCH16, _set(img_res=50), b"image 50 not divisible by patch 16"),
    ("patch_zero", PATCH16, _set(patch=0), b"not divisible by patch 0"),
    ("patch_k", PATCH16, _set(K=764), b"patch mode needs K == 3*patch^2"),
    ("patch_rows", PATCH16, _set(M=19), b"patch mode shape mismatch"),
    ("patch_out_tokens", PATCH16, _set(out_tokens=9), b"patch mode shape mismatch"),
    ("patch_image_misaligned", PATCH16, lambda g: setattr(g, "A", g.A + 4), b"image rows must be 16-byte aligned"),
    ("lora_without_b", {}, _set(lora_t=0x3000, lora_r=4, lora_nseg=3, lora_seg_width=256), b"bad lora args"),
    ("lora_rank_zero", {}, _set(lora_t=0x3000, lora_b=0x4000, lora_nseg=3, lora_seg_width=256), b"bad lora args"),
    ("lora_seg_not_x32", {}, _set(lora_t=0x3000, lora_b=0x4000, lora_r=4, lora_nseg=3, lora_seg_width=260),
     b"lora segment width must be a multiple of 32 and cover N"),
    ("lora_seg_short", {}, _set(lora_t=0x3000, lora_b=0x4000, lora_r=4, lora_nseg=2, lora_seg_width=256),
     b"lora segment width must be a multiple of 32 and cover N"),
]


def _untouched_plan():
    from clipfs import _lib
    plan = _lib.GemmPlan()
    C.memset(C.byref(plan), 0xA5, C.sizeof(plan))
    return plan, bytes(plan)


@pytest.mark.parametrize("name,kw,change,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_plan_refuses_what_the_gemm_refuses(lib, name, kw, change, message):
    """CLIPFS_EINVAL (1) with the entry point's own message, `plan` untouched.  clipfs_gemm_nt refuses before it opens the
    GPU, so the same arguments are put to it here too (A_f16 apart: there it is the other kernel's business)."""
    g = _good(**kw)
    change(g)
    plan, before = _untouched_plan()
    assert lib.clipfs_gemm_plan(C.byref(g), C.byref(plan)) == 1
    said = lib.clipfs_last_error()
    assert message in said, said
    assert bytes(plan) == before
    if name != "a_f16":
        assert lib.clipfs_gemm_nt(C.byref(g), None) == 1 and lib.clipfs_last_error() == said


def test_plan_refuses_null_arguments(lib):
    plan, before = _untouched_plan()
    assert lib.clipfs_gemm_plan(None, C.byref(plan)) == 1 and b"gemm: null args" in lib.clipfs_last_error()
    assert bytes(plan) == before
    assert lib.clipfs_gemm_nt(None, None) == 1 and b"gemm: null args" in lib.clipfs_last_error()
    assert lib.clipfs_gemm_plan(C.byref(_good()), None) == 1 and b"null plan" in lib.clipfs_last_error()


def test_every_refusal_of_the_entry_point_is_reproduced():
    """the messages of gemm_validate_head / gemm_validate in csrc/gemm.hip, one REFUSALS row (or the null test) each"""
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "jittor-clip-fewshot_amd", "csrc", "gemm.hip")).read()
    body = src[src.index("static int gemm_validate_head"):src.index("static GemmSchedule gemm_schedule_of")]
    heads = [m.strip().encode() for m in re.findall(r'"gemm: ([^"%]*)', body)]  # each message up to its first conversion
    assert len(heads) == 19
    said = [r[3] for r in REFUSALS] + [b"null args"]
    for h in heads:
        assert any(h in s or s in h for s in said), h


def test_query_follows_no_pointer(lib):
    """every pointer is an address nobody mapped"""
    from clipfs import _lib
    g = _good()
    g.bias, g.residual, g.ldres, g.aux_out = 0x54, 0x64, 768, 0x74
    g.lora_t, g.lora_b, g.lora_r, g.lora_nseg, g.lora_seg_width = 0x71, 0x81, 8, 1, 768
    assert _lib.gemm_plan(g) == PLAN["per_rank_scratch"].plan
