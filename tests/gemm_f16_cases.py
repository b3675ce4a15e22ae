"""The cases of the f16 x f16 GEMM (csrc/gemm_f16.hip) that the tests cover, in one place: test_gemm_f16_plan.py (CPU)
asserts with clipfs_gemm_f16_plan that the built library sends every row of PLAN_TABLE to the kernels, row ranges and
stream its row claims (for 256 CUs); test_gemm_f16_matrix_gpu.py runs the GPU cases and asserts the same through the
query on the device's own CU count before it looks at a number.

A case is a shape, a layout (leading dimensions), an epilogue variant, optionally one pointer moved 4 bytes off its
16-byte alignment, and optionally one cached tuning aid (those run in a child process: the library reads them once)."""
from collections import namedtuple

CUS = 256                  # compute units of an MI355X: what the table's plans are stated for
LORA_SCALE = 0.5

# ------------------------------------------------------------------ layouts
LAYOUTS = ("tight", "aligned", "reg")


def leading_dims(layout, N, K):
    """(lda, ldb, ldc, ldres).  `aligned` keeps every row 16-byte aligned (the LDS epilogues stay eligible), `reg` has
    ldc % 4 != 0 and ldres % 4 != 0: only the per-lane register epilogue can store such rows."""
    if layout == "tight":
        return K, K, N, N
    if layout == "aligned":
        return K + 8, K + 8, N + 16, N + 24
    assert layout == "reg"
    return K + 8, K + 8, N + 13, N + 21


# ------------------------------------------------------------------ epilogue variants
def _epi(name, out="c32", **kw):
    d = dict(name=name, out=out, alpha=1.0, bias=False, residual=False, act=0, aux=None, lora=None)
    d.update(kw)
    assert d["out"] in ("c32", "both", "c16") and d["aux"] in (None, "f16", "f32")
    assert d["act"] != 2 or d["aux"], "act 2 reads the saved pre-activation"
    return d


# lora = (rank, segments, width kind): "x256" a multiple of 256 (the 256 x 256 kernels accept it), "128odd" 128 * odd
# (they decline: a block tile of 256 columns would straddle two segments)
EPILOGUES = [
    _epi("plain"),
    _epi("c32_c16", out="both"),
    _epi("c16", out="c16"),
    _epi("bias", out="both", bias=True),
    _epi("bias_c16", out="c16", bias=True),
    _epi("alpha_bias", alpha=0.125, bias=True),
    _epi("bias_res", bias=True, residual=True),
    _epi("bias_res_c16", out="both", bias=True, residual=True),
    _epi("act1_aux16", out="c16", bias=True, act=1, aux="f16"),
    _epi("act1_aux16_c32", act=1, aux="f16"),
    _epi("act1_aux32", act=1, aux="f32"),
    _epi("act1_noaux", out="both", act=1),
    _epi("act2_aux16", out="c16", act=2, aux="f16"),
    _epi("act2_aux16_c32", out="both", act=2, aux="f16"),
    _epi("act2_aux32", act=2, aux="f32"),
    _epi("act2_aux32_res", act=2, aux="f32", residual=True),
    _epi("lora3", lora=(3, 1, "x256")),
    _epi("lora16_3seg_c16", out="c16", lora=(16, 3, "x256")),
    _epi("lora17_3seg", out="both", lora=(17, 3, "x256")),
    _epi("lora64", lora=(64, 1, "x256")),
    _epi("lora16_3seg_128odd", lora=(16, 3, "128odd")),
    _epi("lora17_128odd_c16", out="c16", lora=(17, 1, "128odd")),
    _epi("bias_lora17_act1_res", bias=True, lora=(17, 3, "x256"), act=1, aux="f16", residual=True),
    _epi("bias_lora64_act1_res_128odd", out="both", bias=True, lora=(64, 3, "128odd"), act=1, aux="f32", residual=True),
    # alpha != 1 with an adapter: refused (the MFMA-accumulated adapter product would be scaled by alpha)
    _epi("alpha_lora16", alpha=0.5, lora=(16, 1, "x256")),
]
EPI = {e["name"]: e for e in EPILOGUES}
assert len(EPI) == len(EPILOGUES)


def ceil_div(a, b):
    return (a + b - 1) // b


def lora_seg_width(N, nseg, kind):
    """smallest width of its kind with nseg segments covering N"""
    if kind == "x256":
        w = 256 * ceil_div(N, 256 * nseg)
    else:
        k = ceil_div(N, 128 * nseg)
        w = 128 * (k + 1 if k % 2 == 0 else k)
        assert (w // 128) % 2 == 1
    assert w % 128 == 0 and w * nseg >= N
    return w


# ------------------------------------------------------------------ the argument block of a case
POINTERS = ("A16", "B16", "C", "C16", "bias", "residual", "aux", "lora_t", "lora_b")


def fake_pointers(offset=None):
    """Addresses for the host-only plan query, which never follows them: 1 MiB apart, `offset` 4 bytes off"""
    ptr = {name: (i + 1) << 20 for i, name in enumerate(POINTERS)}
    if offset:
        ptr[offset] += 4
    return ptr


def gemm_args(M, N, K, layout, e, ptr):
    """clipfs_gemm_args of one f16 x f16 call; `ptr` maps POINTERS to device addresses"""
    from clipfs import _lib
    g = _lib.new_gemm_args()
    g.M, g.N, g.K = M, N, K
    g.lda, g.ldb, g.ldc, ldres = leading_dims(layout, N, K)
    g.A_f16, g.B_planes, g.b_format = ptr["A16"], ptr["B16"], 2
    g.alpha, g.act = e["alpha"], e["act"]
    if e["out"] in ("c32", "both"):
        g.C = ptr["C"]
    if e["out"] in ("c16", "both"):
        g.C_f16 = ptr["C16"]
    if e["bias"]:
        g.bias = ptr["bias"]
    if e["residual"]:
        g.residual, g.ldres = ptr["residual"], ldres
    if e["aux"]:
        g.aux_f16 = int(e["aux"] == "f16")
        if e["act"] == 1:
            g.aux_out = ptr["aux"]
        elif e["act"] == 2:
            g.aux_in = ptr["aux"]
    if e["lora"]:
        r, nseg, kind = e["lora"]
        g.lora_t, g.lora_b = ptr["lora_t"], ptr["lora_b"]
        g.lora_r, g.lora_nseg, g.lora_seg_width, g.lora_scale = r, nseg, lora_seg_width(N, nseg, kind), LORA_SCALE
    return g


def query_plan(case, ptr=None, cus=CUS):
    """the library's plan for `case` as a tuple of (kernel name, m_begin, m_end, side)"""
    from clipfs import _lib
    g = gemm_args(case.M, case.N, case.K, case.layout, EPI[case.epi], ptr or fake_pointers(case.offset))
    return tuple(_lib.gemm_f16_plan(g, cus))


# ------------------------------------------------------------------ the plan table (256 CUs)
# env: one cached tuning aid "NAME=value" or None;  plan: ((kernel, m_begin, m_end, side stream), ...)
Case = namedtuple("Case", "name M N K layout epi offset env plan")


def _c(name, M, N, K, plan, layout="tight", epi="plain", offset=None, env=None):
    return Case(name, M, N, K, layout, epi, offset, env, tuple(plan))


def _pp(kernel, M, split=None, left="64x128_s2", side=True):
    """the 256 x 256 kernel on [0, split), the leftover rows (if any) as one launch behind it"""
    split = (M // 256) * 256 if split is None else split
    return ((kernel, 0, split, False),) + (((left, split, M, side),) if split < M else ())


PLAN_TABLE = [
    # ---- the nine kernels; 2048 x 2560 is 8 x 10 = 80 tiles of 256 x 256, the fewest the fill rule accepts (>= 77)
    _c("ph16_whole_rounds", 2048, 2560, 128, _pp("ph16", 2048)),
    _c("ph16_wide_f16_result", 2048, 2560, 128, _pp("ph16_wide", 2048), epi="c16"),
    _c("ph32_by_aid", 2048, 2560, 128, _pp("ph32", 2048), env="CLIPFS_F16_PHASED=2"),
    _c("pp_lds_k160", 2048, 2560, 160, _pp("pp_lds", 2048)),
    _c("pp_lds_k224_leftover", 2088, 2560, 224, _pp("pp_lds", 2088), epi="c16"),
    _c("pp_lds_by_aid_k128", 2048, 2560, 128, _pp("pp_lds", 2048), env="CLIPFS_F16_PHASED=0"),
    _c("pp_reg_fp32_aux", 2048, 2560, 128, _pp("pp_reg", 2048), epi="act1_aux32"),
    _c("pp_reg_by_aid", 2048, 2560, 128, _pp("pp_reg", 2048), env="CLIPFS_F16_EPILOGUE=0"),
    _c("k64_tiny_64x128", 257, 403, 64, (("64x128", 0, 257, False),)),
    # ---- leftover rows beside the 256 x 256 launch
    _c("leftover_1_row_side", 2049, 2560, 128, _pp("ph16", 2049)),
    _c("leftover_40_rows_side", 2088, 2560, 192, _pp("ph16", 2088)),
    _c("leftover_255_rows_side", 2303, 2568, 448, _pp("ph16_wide", 2303), epi="c16"),
    _c("leftover_same_stream_by_aid", 2088, 2560, 128, _pp("ph16", 2088, left="64x128", side=False),
       env="CLIPFS_F16_SIDE=0"),
    # 3 x 96 = 288 tiles, 32 beyond a round of 256 (< 30 %): two m-blocks stay, 328 rows are 6 x 192 = 1152 small tiles
    # > 1024, so the side stream gets the 4-wave dispatch: 3 x 192 tiles of 128 rows >= 512.  41 MB of f16 output.
    _c("leftover_over_1024_tiles_4wave_on_side", 840, 24576, 128, _pp("ph16_wide", 840, split=512, left="128x128"), epi="c16"),
    # ---- the 256 x 256 path declined
    _c("declined_k96", 2048, 2560, 96, (("64x128", 0, 2048, False),)),
    _c("declined_seg_128odd", 2088, 2560, 128, (("64x128", 0, 2088, False),), epi="lora16_3seg_128odd"),
    _c("accepted_seg_x256", 2088, 2560, 128, _pp("ph16", 2088), epi="lora17_3seg"),
    # 8 x 9 = 72 tiles: 7200 < 256 * 30
    _c("declined_fill_rule", 2048, 2304, 128, (("64x128", 0, 2048, False),)),
    # 2 x 130 = 260 tiles, 4 beyond a round of 256 (< 30 %): 256 tiles are ONE whole m-block, and 256 of 767 rows is
    # less than 60 %, so everything goes to the 4-wave kernels (CPU only: not among the GPU cases)
    _c("declined_60_percent", 767, 33280, 128, (("256x128", 0, 767, False),), epi="c16"),
    # ---- dispatch_rows_4wave: small-problem rule (N = 2048: 16 column blocks) and the peel
    _c("4wave_small_64x128", 3968, 2048, 64, (("64x128", 0, 3968, False),)),     # 31 x 16 = 496 < 512 tiles of 128 rows
    _c("4wave_small_128x128", 4096, 2048, 64, (("128x128", 0, 4096, False),)),   # 32 x 16 = 512
    _c("4wave_256x128", 8192, 2048, 64, (("256x128", 0, 8192, False),)),         # 32 x 16 = 512 tiles of 256 rows
    # 34 x 16 = 544 tiles, 32 beyond the round (<= 64): two m-blocks are peeled onto 64-row tiles
    _c("4wave_peel", 8488, 2048, 64, (("256x128", 0, 8192, False), ("64x128", 8192, 8488, False))),
    _c("tile_aid_4_every_row_pp", 300, 2560, 128, (("ph16", 0, 300, False),), env="CLIPFS_F16_TILE=4"),
    _c("tile_aid_4_ragged_m", 2088, 2560, 128, (("ph16_wide", 0, 2088, False),), epi="c16", env="CLIPFS_F16_TILE=4"),
    _c("tile_aid_4_two_phase", 2088, 2560, 160, (("pp_lds", 0, 2088, False),), env="CLIPFS_F16_TILE=4"),
    # ---- register / LDS / wide for ONE shape (2088 x 2560 x 128): leading dimensions and pointer alignment decide
    _c("epi_wide_tight", 2088, 2560, 128, _pp("ph16_wide", 2088), epi="bias_c16"),
    _c("epi_wide_aligned_ld", 2088, 2560, 128, _pp("ph16_wide", 2088), layout="aligned", epi="bias_c16"),
    _c("epi_reg_ldc_odd", 2088, 2560, 128, _pp("pp_reg", 2088), layout="reg", epi="bias_c16"),
    _c("epi_reg_bias_off_16", 2088, 2560, 128, _pp("pp_reg", 2088), epi="bias_c16", offset="bias"),
    _c("epi_lds_fp32_result", 2088, 2560, 128, _pp("ph16", 2088), epi="bias"),
    _c("epi_lds_residual", 2088, 2560, 128, _pp("ph16", 2088), layout="aligned", epi="bias_res"),
    _c("epi_reg_ldres_odd", 2088, 2560, 128, _pp("pp_reg", 2088), layout="reg", epi="bias_res"),
    _c("epi_reg_c_off_16", 2088, 2560, 128, _pp("pp_reg", 2088), epi="bias", offset="C"),
    _c("epi_reg_residual_off_16", 2088, 2560, 128, _pp("pp_reg", 2088), epi="bias_res", offset="residual"),
    _c("epi_wide_n_plus_8", 2088, 2568, 128, _pp("ph16_wide", 2088), epi="act1_aux16"),
    _c("epi_lds_n_plus_4", 2088, 2564, 128, _pp("ph16", 2088), epi="act1_aux16"),
    _c("epi_reg_n_plus_2", 2088, 2562, 128, _pp("pp_reg", 2088), epi="act1_aux16"),
    _c("epi_reg_act2_with_residual", 2088, 2560, 128, _pp("pp_reg", 2088), epi="act2_aux32_res"),
]
PLAN = {c.name: c for c in PLAN_TABLE}
assert len(PLAN) == len(PLAN_TABLE)
KERNELS = ("64x128", "64x128_s2", "128x128", "256x128", "pp_reg", "pp_lds", "ph16", "ph16_wide", "ph32")


# ------------------------------------------------------------------ rows under a cached aid: asked in a child process
def aids():
    return sorted({c.env for c in PLAN_TABLE if c.env})


def child_env(aid):
    import os
    name, value = aid.split("=")
    env = {k: v for k, v in os.environ.items() if not k.startswith("CLIPFS_F16_")}
    env[name] = value
    return env


def child_command(call):
    """argv of a fresh interpreter that runs `call` (an expression on this module, imported as `cases`)"""
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    pkg = os.path.join(os.path.dirname(here), "jittor-clip-fewshot_amd")
    code = f"import sys; sys.path[:0] = [{here!r}, {pkg!r}]; import gemm_f16_cases as cases; {call}"
    return [sys.executable, "-c", code]


def print_plans(aid):
    """child side: one JSON line with the plan of every row stated for `aid`"""
    import json
    print("PLANS " + json.dumps({c.name: query_plan(c) for c in PLAN_TABLE if c.env == aid}))


# ------------------------------------------------------------------ the GPU cases (test_gemm_f16_matrix_gpu.py)
def pp_kernel_for(N, K, layout, e, offset=None, aid=None):
    """The 256 x 256 kernel a case is MEANT for, from the conditions csrc/gemm_f16.hip documents: the register epilogue
    when a row of C / the residual or one of the pointers is not 16-byte aligned, for an fp32 pre-activation and for act 2
    with a residual; else 2-phase when K % 64 != 0; else phased, 8 columns per thread for an f16-only result without a
    residual whose rows are 16-byte aligned as f16."""
    _, _, ldc, ldres = leading_dims(layout, N, K)
    reg = (N % 4 or ldc % 4 or (e["residual"] and ldres % 4) or offset or e["aux"] == "f32" or
           (e["residual"] and e["act"] == 2) or aid == "CLIPFS_F16_EPILOGUE=0")
    if reg:
        return "pp_reg"
    if K % 64 or K < 128 or aid == "CLIPFS_F16_PHASED=0":
        return "pp_lds"
    if aid == "CLIPFS_F16_PHASED=2":
        return "ph32"
    return "ph16_wide" if e["out"] == "c16" and not e["residual"] and N % 8 == 0 and ldc % 8 == 0 else "ph16"


def _gpu(M, N, K, layout, epi, offset=None, aid=None, plan=None):
    e = EPI[epi]
    if plan is None:
        if K < 128 or (e["lora"] and e["lora"][2] == "128odd"):
            assert ceil_div(M, 128) * ceil_div(N, 128) < 512
            plan = (("64x128", 0, M, False),)
        elif aid == "CLIPFS_F16_TILE=4":
            plan = ((pp_kernel_for(N, K, layout, e, offset), 0, M, False),)
        else:
            tiles = (M // 256) * ceil_div(N, 256)
            assert CUS * 30 <= tiles * 100 and tiles <= CUS and ((M - M // 256 * 256 + 63) // 64) * ceil_div(N, 128) <= 1024
            plan = _pp(pp_kernel_for(N, K, layout, e, offset, aid), M)
            if aid == "CLIPFS_F16_SIDE=0" and len(plan) == 2:
                plan = (plan[0], ("64x128", plan[1][1], M, False))
    kernels = "+".join(l[0] for l in plan)
    name = f"{kernels}-{M}x{N}x{K}-{layout}-{epi}" + (f"-{offset}_off_4_bytes" if offset else "")
    return Case(name, M, N, K, layout, epi, offset, aid, tuple(plan))


RUN_EPILOGUES = [e["name"] for e in EPILOGUES if e["name"] != "alpha_lora16"]   # that one is refused: its own test


def _rotate(shapes, epis, layouts=LAYOUTS):
    """every shape once; epilogues and layouts advance so that over the list each epilogue meets each layout"""
    return [_gpu(M, N, K, layouts[(i // len(epis) + i) % len(layouts)], epis[(i * 7) % len(epis)])
            for i, (M, N, K) in enumerate(shapes)]


SMALL_M, SMALL_N, SMALL_K = (1, 63, 64, 65, 255, 257), (8, 128, 136, 403), (32, 64, 96)
BIG_M, BIG_N = (2048, 2049, 2088, 2303), (2560, 2568, 2564, 2562)
PHASED_K, TWO_PHASE_K = (128, 192, 256, 448), (160, 224)
SWEEP_EPILOGUES = ["c16", "act1_aux16", "bias_res", "act2_aux16_c32", "lora16_3seg_c16", "c32_c16", "act2_aux16"]

GPU_CASES = (
    # the 64 x 128 kernel (K < 128, few tiles): every small shape once, and every epilogue in every layout on the one
    # shape with whole AND ragged tiles in both directions
    _rotate([(M, N, K) for K in SMALL_K for M in SMALL_M for N in SMALL_N], RUN_EPILOGUES)
    + [_gpu(257, 403, 96, layout, epi) for epi in RUN_EPILOGUES for layout in LAYOUTS]
    # 256 x 256 kernels: every epilogue in every layout at one phased shape with leftover rows ...
    + [_gpu(2088, 2560, 128, layout, epi) for epi in RUN_EPILOGUES for layout in LAYOUTS]
    # ... the 2-phase kernel on those the LDS epilogue treats differently ...
    + [_gpu(2088, 2560, 160, layout, epi) for layout in ("tight", "aligned")
       for epi in ("plain", "c16", "bias_res_c16", "act1_aux16", "act2_aux16_c32", "lora3", "lora17_3seg", "lora64",
                   "bias_lora17_act1_res")]
    + [_gpu(2088, 2560, 160, "reg", epi) for epi in ("c16", "bias_lora17_act1_res")]
    # ... every M x N of the big shapes at one phased and one 2-phase K, the diagonal at the other K
    + _rotate([(M, N, K) for K in (128, 160) for M in BIG_M for N in BIG_N], SWEEP_EPILOGUES)
    + _rotate([(M, N, K) for K in (192, 256, 448, 224) for M, N in zip(BIG_M, BIG_N)], SWEEP_EPILOGUES[::-1])
    # one pointer 4 bytes off its 16-byte alignment: the register epilogue
    + [_gpu(2088, 2560, 128, "tight", "bias", offset="C"), _gpu(2088, 2560, 128, "tight", "bias_c16", offset="bias"),
       _gpu(2088, 2560, 128, "aligned", "bias_res", offset="residual"), _gpu(257, 403, 96, "tight", "bias_res", offset="C")]
    # the 256 x 256 path declined by the fill rule; leftover rows of more than 1024 small tiles (128 x 128 on the side stream)
    + [_gpu(2048, 2304, 128, "aligned", "bias_res_c16", plan=PLAN["declined_fill_rule"].plan),
       _gpu(840, 24576, 128, "aligned", "act1_aux16", plan=PLAN["leftover_over_1024_tiles_4wave_on_side"].plan)]
    # the other 4-wave kernels and the peel need 512 tiles: one case per layout
    + [_gpu(M, 2048, 64, layout, epi, plan=PLAN[row].plan)
       for M, row, epis in ((4096, "4wave_small_128x128", ("bias_res_c16", "act1_aux32", "lora17_3seg")),
                            (8192, "4wave_256x128", ("act2_aux16_c32", "bias_lora64_act1_res_128odd", "c16")),
                            (8488, "4wave_peel", ("act1_aux16", "alpha_bias", "act2_aux32_res")))
       for layout, epi in zip(LAYOUTS, epis)]
)

# under a cached aid, each list in one child process
AID_CASES = {
    "CLIPFS_F16_PHASED=2": [_gpu(2088, 2560, 128, lay, epi, aid="CLIPFS_F16_PHASED=2") for lay, epi in (
        ("tight", "plain"), ("aligned", "c16"), ("aligned", "bias_res_c16"), ("tight", "act1_aux16"),
        ("tight", "act2_aux16_c32"), ("tight", "lora17_3seg"), ("aligned", "bias_lora17_act1_res"))]
    + [_gpu(2303, 2568, 448, "tight", "lora64", aid="CLIPFS_F16_PHASED=2")],
    "CLIPFS_F16_PHASED=0": [_gpu(2088, 2560, K, lay, epi, aid="CLIPFS_F16_PHASED=0") for K, lay, epi in (
        (128, "tight", "plain"), (128, "aligned", "c16"), (192, "tight", "lora17_3seg"),
        (192, "aligned", "bias_lora17_act1_res"), (256, "tight", "act2_aux16"))],
    "CLIPFS_F16_EPILOGUE=0": [_gpu(2088, 2560, 128, lay, epi, aid="CLIPFS_F16_EPILOGUE=0") for lay, epi in (
        ("tight", "c16"), ("aligned", "bias_res_c16"), ("tight", "act1_aux16"), ("aligned", "act2_aux16_c32"),
        ("tight", "bias_lora17_act1_res"))],
    "CLIPFS_F16_SIDE=0": [_gpu(2088, 2560, 128, "tight", "plain", aid="CLIPFS_F16_SIDE=0"),
                          _gpu(2303, 2568, 448, "aligned", "c16", aid="CLIPFS_F16_SIDE=0"),
                          _gpu(2049, 2564, 160, "tight", "bias_lora17_act1_res", aid="CLIPFS_F16_SIDE=0")],
    # the 256 x 256 kernels on a ragged last m-block: their row clamps
    "CLIPFS_F16_TILE=4": [_gpu(M, 2560, K, lay, epi, aid="CLIPFS_F16_TILE=4") for M in (300, 2088) for K, lay, epi in (
        (128, "tight", "plain"), (128, "aligned", "c16"), (128, "aligned", "bias_res_c16"), (128, "tight", "act2_aux16"),
        (128, "tight", "lora17_3seg"), (160, "tight", "act1_aux16"), (160, "aligned", "bias_lora17_act1_res"),
        (128, "reg", "bias_res_c16"), (128, "tight", "act1_aux32"))],
}
GPU_CASES = list({c.name: c for c in GPU_CASES}.values())   # a rotated shape may repeat a case of a full block
