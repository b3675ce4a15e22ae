"""The plan table of the exact fp32 / 16-bit-plane GEMM dispatch (csrc/gemm.hip, gemm_schedule): for every row the FULL
struct clipfs_gemm_plan that clipfs_gemm_plan -- the function clipfs_gemm_nt executes -- must answer.  test_gemm_plan.py
(CPU) asserts it.  The counterpart of gemm_f16_cases.py; pointers are fake aligned addresses the query never follows.

The rows are the hand-derived ones of the issue that asked for the plan, every row of gemm_matrix_cases.py with and
without scratch, the 16-bit-plane shapes in both formats, the patch modes, and one row per tuning aid.  The arithmetic
behind a row stands beside it.  Every hand-derived value of the issue was confirmed by the query; none had to be
corrected.  What the issue left open and the query settled: the patch-32 and generic kernels report tile_rows 64 and
want_splits 1 (the shape-only queries still answer 32 rows / 8 slices for the 98-row patch embed), and the mixed launch
reports tile_rows 32."""
from collections import namedtuple

from gemm_matrix_cases import BK, PLANE_SHAPES, SCHEDULE_CLASSES, ceil_div

KERNELS = ("nt64", "nt64_reg", "nt32", "mixed", "patch32", "generic", "planes64", "planes128")
POINTERS = ("A", "B", "C", "planes", "workspace", "counters")
LDS64, LDS32 = 57408, 49216   # 2 stages x (64 | 32 + 128) rows x 128 B + 8 KiB pad + 64 B flag word
PLAN_FIELDS = ("kernel", "planes", "tile_rows", "splits", "want_splits", "mix_rows64", "gm", "grid", "block", "lds_bytes",
               "workspace_floats", "counter_ints")

# scratch: "full" (what the shape-only queries ask for), "none", "misaligned" (workspace 4 bytes off), "few_counters"
# planes: None | "bf16x3" | "f16_plane";  patch: None | (images, resolution, patch);  env: one cached aid or None
Case = namedtuple("Case", "name M N K scratch planes ldb_pad patch env plan")


def plan(kernel, tile_rows, grid, lds, splits=1, want=None, ws=0, cnt=0, mix=0, planes=0, gm=8):
    want = splits if want is None else want
    return dict(kernel=kernel, planes=planes, tile_rows=tile_rows, splits=splits, want_splits=want, mix_rows64=mix, gm=gm,
                grid=grid, block=256, lds_bytes=lds, workspace_floats=ws, counter_ints=cnt)


def _c(name, M, N, K, plan_, scratch="full", planes=None, ldb_pad=False, patch=None, env=None):
    return Case(name, M, N, K, scratch, planes, ldb_pad, patch, env, plan_)


def _patch(name, B, R, ps, N, plan_):
    return _c(name, B * (R // ps) ** 2, N, 3 * ps * ps, plan_, patch=(B, R, ps))


def _class_rows(c):
    """a SCHEDULE_CLASSES row with and without scratch: the generic kernel for a K tail (64-row tiles, never split), else
    the row's tile height and split factor"""
    if c.K % BK:
        full = bare = plan("generic", 64, ceil_div(c.M, 64) * ceil_div(c.N, 128), LDS64)
    else:
        kernel, lds = ("nt32", LDS32) if c.tile_rows == 32 else ("nt64", LDS64)
        tiles = ceil_div(c.M, c.tile_rows) * ceil_div(c.N, 128)
        need = dict(ws=c.S * tiles * c.tile_rows * 128, cnt=tiles) if c.S > 1 else {}
        full = plan(kernel, c.tile_rows, tiles * c.S, lds, splits=c.S, **need)
        bare = plan(kernel, c.tile_rows, tiles, lds, splits=1, want=c.S, **need)
    return [_c(f"class_{c.name}", c.M, c.N, c.K, full), _c(f"class_{c.name}_bare", c.M, c.N, c.K, bare, scratch="none")]


def _plane_rows(s):
    """64 x 128 tiles, 128 x 128 from 1024 such tiles on; two stages of (rows + 128) x 64 B per 16-bit plane"""
    rows = 128 if s.big_tile else 64
    kernel, grid = ("planes128" if s.big_tile else "planes64"), ceil_div(s.M, rows) * ceil_div(s.N, 128)
    return [_c(f"{fmt}_{s.name}", s.M, s.N, s.K, plan(kernel, rows, grid, 2 * npl * (rows + 128) * 64, planes=npl), planes=fmt)
            for fmt, npl in (("bf16x3", 2), ("f16_plane", 1))]


_PER_RANK = dict(ws=3 * 150 * 64 * 128, cnt=150)   # 25 x 6 tiles of 64 x 128, three K slices

PLAN_TABLE = [
    # ---- the per-rank shape: 150 tiles < 384, ceil(448 / 150) = 3 slices of 24 K-steps
    _c("per_rank_scratch", 1600, 768, 768, plan("nt64", 64, 450, LDS64, splits=3, **_PER_RANK)),
    _c("per_rank_no_workspace", 1600, 768, 768, plan("nt64", 64, 150, LDS64, want=3, **_PER_RANK), scratch="none"),
    _c("per_rank_misaligned_workspace", 1600, 768, 768, plan("nt64", 64, 150, LDS64, want=3, **_PER_RANK), scratch="misaligned"),
    _c("per_rank_few_counters", 1600, 768, 768, plan("nt64", 64, 150, LDS64, want=3, **_PER_RANK), scratch="few_counters"),
    # 22 x 4 tiles of 32 rows (one round at 1.08 x 32 beats one round of 64); 4 K-steps: too short to cut
    _c("tile32_unsplit", 700, 480, 128, plan("nt32", 32, 88, LDS32)),
    # one round of the 512 slots as 64-row tiles = 128 m-blocks = 8192 rows; ceil(1556 / 32) x 4 = 196 tiles behind them
    _c("band_bench_rows", 9748, 512, 512, plan("mixed", 32, 708, LDS64, mix=8192)),
    # ---- K % 32 != 0: the generic kernel, 64-row tiles, whatever clipfs_gemm_tile_rows answers
    _c("ktail_generic", 1300, 1000, 100, plan("generic", 64, 21 * 8, LDS64)),
    _c("ktail_tiny", 50, 64, 100, plan("generic", 64, 1, LDS64)),
    # ---- patch mode: ViT-B/32 on two 224-pixel images (2 x 6 tiles, unsplit), the other patch sizes on the generic kernel
    _patch("patch32_vit_b32", 2, 224, 32, 768, plan("patch32", 64, 12, LDS64)),
    _patch("patch16", 2, 48, 16, 96, plan("generic", 64, 1, LDS64)),
    _patch("patch14", 2, 28, 14, 200, plan("generic", 64, 2, LDS64)),
    # ---- planes with ldb != K fall to the fp32 kernels: 32 x 4 tiles of 32 rows, ceil(448 / 128) = 4 > 8 K-steps / 4 = 2
    _c("bf16x3_padded_ldb_exact", 1000, 480, 256, plan("nt32", 32, 256, LDS32, splits=2, ws=2 * 128 * 32 * 128, cnt=128),
       planes="bf16x3", ldb_pad=True),
    _c("f16_plane_padded_ldb_exact", 1000, 480, 256, plan("nt32", 32, 256, LDS32, splits=2, ws=2 * 128 * 32 * 128, cnt=128),
       planes="f16_plane", ldb_pad=True),
    # planes never split, whatever the scratch
    _c("bf16x3_per_rank_unsplit", 1600, 768, 768, plan("planes64", 64, 150, 49152, planes=2), planes="bf16x3"),
    # ---- one row per tuning aid (each is read once per process: asked in a fresh child)
    _c("aid_bm64", 700, 480, 128, plan("nt64", 64, 11 * 4, LDS64), env="CLIPFS_GEMM_BM=64"),
    # 40 x 10 tiles of 64 rows, 9 K-steps >= 2 x 2
    _c("aid_splits2", 2500, 1200, 288, plan("nt64", 64, 800, LDS64, splits=2, ws=2 * 400 * 64 * 128, cnt=400), env="CLIPFS_GEMM_SPLITS=2"),
    _c("aid_gm4", 2500, 1200, 288, plan("nt64", 64, 400, LDS64, gm=4), env="CLIPFS_GEMM_GM=4"),
    _c("aid_lds_pad0", 2500, 1200, 288, plan("nt64", 64, 400, LDS64 - 8192), env="CLIPFS_GEMM_LDS_PAD=0"),
    _c("aid_glds0_register_staging", 2500, 1200, 288, plan("nt64_reg", 64, 400, LDS64), env="CLIPFS_GEMM_GLDS=0"),
    # the mixed launch exists with LDS-DMA staging only: 305 x 4 tiles of 32 rows
    _c("aid_glds0_no_band", 9748, 512, 512, plan("nt32", 32, 1220, LDS32), env="CLIPFS_GEMM_GLDS=0"),
    _c("aid_bf16_tile1", 300, 403, 96, plan("planes128", 128, 3 * 4, 2 * 2 * 256 * 64, planes=2), planes="bf16x3", env="CLIPFS_BF16_TILE=1"),
] + [r for c in SCHEDULE_CLASSES for r in _class_rows(c)] + [r for s in PLANE_SHAPES for r in _plane_rows(s)]
PLAN = {c.name: c for c in PLAN_TABLE}
assert len(PLAN) == len(PLAN_TABLE)

AID_PREFIXES = ("CLIPFS_GEMM_", "CLIPFS_BF16_")


# ------------------------------------------------------------------ arguments and the query
def fake_pointers():
    """Addresses for the host-only plan query, which never follows them: 16-byte aligned, 1 GiB apart"""
    return {name: (i + 1) << 30 for i, name in enumerate(POINTERS)}


def gemm_args(M, N, K, *, scratch="full", planes=None, ldb_pad=False, patch=None, ptr=None):
    """clipfs_gemm_args of one exact fp32 / 16-bit-plane call on fake pointers; `scratch` as in Case"""
    from clipfs import _lib
    lib = _lib.load()
    ptr = ptr or fake_pointers()
    g = _lib.new_gemm_args()
    g.A, g.B, g.C = ptr["A"], ptr["B"], ptr["C"]
    g.M, g.N, g.K = M, N, K
    g.lda, g.ldb, g.ldc = (0 if patch else K), (K + 4 if ldb_pad else K), N
    g.alpha = 1.0
    if patch:
        g.a_mode = 1
        g.img_res, g.patch, g.out_tokens = patch[1], patch[2], (patch[1] // patch[2]) ** 2 + 1
    if planes:
        g.B_planes, g.b_format = ptr["planes"], (1 if planes == "bf16x3" else 2)
    if scratch != "none":
        g.workspace, g.workspace_floats = ptr["workspace"] + (4 if scratch == "misaligned" else 0), lib.clipfs_gemm_workspace_floats(M, N, K)
        g.counters, g.counters_ints = ptr["counters"], lib.clipfs_gemm_counter_ints(M, N, K) - (1 if scratch == "few_counters" else 0)
    return g


def query_plan(case):
    from clipfs import _lib
    return _lib.gemm_plan(gemm_args(case.M, case.N, case.K, scratch=case.scratch, planes=case.planes, ldb_pad=case.ldb_pad,
                                    patch=case.patch))


# ------------------------------------------------------------------ rows under a cached aid: one fresh child per aid
def aids():
    return sorted({c.env for c in PLAN_TABLE if c.env})


def child_env(aid):
    import os
    name, value = aid.split("=")
    env = {k: v for k, v in os.environ.items() if not k.startswith(AID_PREFIXES)}
    env[name] = value
    return env


def child_command(call):
    """argv of a fresh interpreter that runs `call` (an expression on this module, imported as `cases`)"""
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    pkg = os.path.join(os.path.dirname(here), "jittor-clip-fewshot_amd")
    code = f"import sys; sys.path[:0] = [{here!r}, {pkg!r}]; import gemm_plan_cases as cases; {call}"
    return [sys.executable, "-c", code]


def print_plans(aid):
    """child side: one JSON line with the plan of every row stated for `aid`"""
    import json
    print("PLANS " + json.dumps({c.name: query_plan(c) for c in PLAN_TABLE if c.env == aid}))
