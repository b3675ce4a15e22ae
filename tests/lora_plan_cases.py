"""The case table of tests/test_lora_plan.py: what clipfs_lora_plan -- the function clipfs_lora_down, _bwd, _bwd_xact and
_bwd_f16dy execute -- must answer, row by row, and a short restatement of the two slice rules for the grid test.

Launch geometry the rows state (matrix-core family, backward; G = ceil(r / 16), nb = nseg segw r, na = nseg r width):
  dB partials || dt   ceil(nseg segw / 256) slices_b + ceil(rows / 16) blocks of 256
  dA partials || dx   ceil(width / 256) slices_a + ceil(rows / 16) blocks of 256
  both slice sums     ceil(nb / 64) + ceil(na / 64) blocks of 1024
Row family: dt, dB partials, sum, dA partials, sum, dx -- blocks of 256, 256, 1024, 64, 1024, 256."""
from collections import namedtuple


def ceil_div(a, b):
    return -(-a // b)


def al4(n):
    return (n + 3) & ~3


# ------------------------------------------------------------------ the slice rules, restated
def row_slice_rows(rows):
    sr = 64
    while sr > 8 and ceil_div(rows, sr) < 256:
        sr >>= 1
    return sr


def mfma_slice_rows(rows, col_groups):
    sr = 2048
    while sr > 64 and col_groups * ceil_div(rows, sr) < 6144:
        sr >>= 1
    return sr


def slices(family, rows, width, segw, r, nseg):
    """(sr_b, slices_b, sr_a, slices_a) of a backward with gradient slots"""
    if family == "row":
        sr_b = sr_a = row_slice_rows(rows)
    else:
        g = ceil_div(r, 16)
        sr_b, sr_a = mfma_slice_rows(rows, nseg * segw // 64 * g), mfma_slice_rows(rows, width // 64 * g)
    return sr_b, ceil_div(rows, sr_b), sr_a, ceil_div(rows, sr_a)


def work_floats(family, rows, width, segw, r, nseg):
    _, sb, _, sa = slices(family, rows, width, segw, r, nseg)
    return al4(sb * nseg * segw * r) + sa * nseg * r * width


def work_bound(rows, width, segw, r, nseg):
    """clipfs_lora_bwd_work_floats2: over the families that may take the call -- above r = 16 the matrix-core family
    alone, up to 16 either, of which the row family (slices of at most 64 rows) needs the most -- plus 64."""
    return work_floats("mfma" if r > 16 else "row", rows, width, segw, r, nseg) + 64


# ------------------------------------------------------------------ the rows
# want: a dict of plan fields (every one must match), or a substring of the refusal's message;  env: a cached aid or None
Case = namedtuple("Case", "name op rows width segw r nseg flags env want bound")

ROW_BLOCKS = (256, 256, 1024, 64, 1024, 256)


def mfma(rows, width, segw, r, nseg, g_rq, sl, work, grids):
    sr_b, sb, sr_a, sa = sl
    return dict(family="mfma", groups=g_rq[0], rq=g_rq[1], sr_b=sr_b, slices_b=sb, sr_a=sr_a, slices_a=sa, work_floats=work,
                part_a_offset=al4(sb * nseg * segw * r), launches=tuple((g, 1, b) for g, b in zip(grids, (256, 256, 1024))))


def row(rows, width, segw, r, nseg, sl, work, grids):
    sr, s = sl
    return dict(family="row", groups=0, rq=0, sr_b=sr, slices_b=s, sr_a=sr, slices_a=s, work_floats=work,
                part_a_offset=al4(s * nseg * segw * r),
                launches=tuple((g if isinstance(g, tuple) else (g, 1)) + (b,) for g, b in zip(grids, ROW_BLOCKS)))


# (rows, width, segw, r, nseg), plan, bound (clipfs_lora_bwd_work_floats2), extra flags, operation
_NAMED = [
    ("image_r4", (12800, 768, 768, 4, 3), mfma, ((1, 1), (64, 200, 64, 200), 3_686_400, (2600, 1400, 288)), 7_372_864, {}, "bwd"),
    ("text_r4", (31031, 512, 512, 4, 3), mfma, ((1, 1), (64, 485, 64, 485), 5_959_680, (4850, 2910, 192)), 5_959_744, {}, "bwd"),
    ("l14_r16", (32896, 1024, 1024, 16, 3), mfma, ((1, 4), (256, 129, 64, 514), 31_604_736, (3604, 4112, 1536)), 50_528_320, {}, "bwd"),
    ("l14_r16_f16dy", (32896, 1024, 1024, 16, 3), mfma, ((1, 4), (256, 129, 64, 514), 31_604_736, (3604, 4112, 1536)), 50_528_320, {},
     "bwd_f16dy"),
    ("r17", (45, 512, 512, 17, 3), mfma, ((2, 8), (64, 1, 64, 1), 52_224, (9, 5, 816)), 52_288, {}, "bwd"),
    ("r48", (333, 512, 512, 48, 3), mfma, ((3, 12), (64, 6, 64, 6), 884_736, (57, 33, 2304)), 884_800, {}, "bwd"),
    ("r64", (1100, 768, 768, 64, 3), mfma, ((4, 16), (64, 18, 64, 18), 5_308_416, (231, 123, 4608)), 5_308_480, {}, "bwd"),
    ("c_fc", (12800, 768, 3072, 4, 1), mfma, ((1, 1), (64, 200, 64, 200), 3_072_000, (3200, 1400, 240)), 6_144_064, {}, "bwd"),
    ("c_proj_x_act", (12800, 3072, 768, 4, 1), mfma, ((1, 1), (64, 200, 64, 200), 3_072_000, (1400, 3200, 240)), 6_144_064,
     dict(x_act=True), "bwd"),
    ("per_rank", (1600, 768, 768, 4, 3), mfma, ((1, 1), (64, 25, 64, 25), 460_800, (325, 175, 288)), 3_686_464, {}, "bwd"),
    ("tiny_r1", (7, 512, 512, 1, 1), mfma, ((1, 1), (64, 1, 64, 1), 1_024, (3, 3, 16)), 1_088, {}, "bwd"),
    ("rect_r64", (300, 128, 512, 64, 1), mfma, ((4, 16), (64, 5, 64, 5), 204_800, (29, 24, 640)), 204_864, {}, "bwd"),
    ("row_192", (150, 192, 192, 2, 3), row, ((8, 19), 43_776, (38, (3, 19), 18, (1, 19), 18, 38)), 43_840, {}, "bwd"),
    ("row_rect", (300, 64, 256, 4, 1), row, ((8, 38), 48_640, (75, (1, 38), 16, (1, 38), 4, 75)), 48_704, {}, "bwd"),
]


def _c(name, op, shape, want, env=None, bound=None, **flags):
    return Case(name, op, *shape, tuple(sorted(flags.items())), env, want, bound)


def _under_aid(name, shape, make, args, flags, op, aid):
    """the same row under CLIPFS_LORA_MFMA=0: the row family up to r = 16 (not for an f16 dy), a refusal above"""
    if op == "bwd_f16dy":
        want = "outside the matrix-core kernels (switched off by CLIPFS_LORA_MFMA=0)"
    elif shape[3] > 16:
        want = f"rank {shape[3]} unsupported"
    else:
        sl = slices("row", *shape)
        nb, na = shape[4] * shape[2] * shape[3], shape[4] * shape[3] * shape[1]
        rows4 = ceil_div(shape[0], 4)
        want = row(*shape, (sl[0], sl[1]), work_floats("row", *shape),
                   (rows4, (ceil_div(shape[4] * shape[2], 256), sl[1]), ceil_div(nb, 64), (ceil_div(shape[1] // 4, 64), sl[1]),
                    ceil_div(na, 64), rows4))
    return _c(f"{name}_{aid}", op, shape, want, env=aid, **flags)


_OK3 = [(w, r) for w in (512, 768, 1024) for r in (4, 17, 64)]
_COVER = dict(keep_bits_ok=1, f16dy_ok=1)
_NOT = dict(keep_bits_ok=0, f16dy_ok=0)

TABLE = (
    [_c(name, op, shape, make(*shape, *args), bound=bound, **flags) for name, shape, make, args, bound, flags, op in _NAMED] +
    # frozen adapter: no partial products, no slice sums, nothing written to work
    [_c("frozen_dx", "bwd", (333, 512, 512, 48, 3), dict(family="mfma", slices_b=0, slices_a=0, work_floats=0, part_a_offset=0,
                                                         launches=((21, 1, 256), (21, 1, 256))), frozen=True),
     _c("frozen_no_dx", "bwd", (333, 512, 512, 48, 3), dict(family="mfma", slices_b=0, slices_a=0, launches=((21, 1, 256),)),
        frozen=True, dx=False),
     _c("no_dx", "bwd", (333, 512, 512, 48, 3), dict(family="mfma", slices_a=6, launches=((57, 1, 256), (12, 1, 256), (2304, 1, 1024))),
        dx=False),
     _c("row_frozen_dx", "bwd", (150, 192, 192, 2, 3), dict(family="row", slices_b=0, slices_a=0, work_floats=0,
                                                            launches=((38, 1, 256), (38, 1, 256))), frozen=True),
     _c("row_frozen_no_dx", "bwd", (150, 192, 192, 2, 3), dict(family="row", launches=((38, 1, 256),)), frozen=True, dx=False)] +
    # down-projection: 16 rows per block on the matrix cores, one wave per row (4 per block) elsewhere
    [_c("down_mfma", "down", (12800, 768, 768, 4, 3), dict(family="mfma", groups=1, rq=0, launches=((800, 1, 256),))),
     _c("down_mfma_r64", "down", (45, 512, 512, 64, 3), dict(family="mfma", groups=4, launches=((3, 1, 256),))),
     _c("down_mfma_4096", "down", (45, 4096, 4096, 4, 1), dict(family="mfma", groups=1, launches=((3, 1, 256),))),
     _c("down_row_192", "down", (150, 192, 192, 2, 3), dict(family="row", groups=0, launches=((38, 1, 256),))),
     _c("down_nseg2", "down", (45, 512, 512, 4, 2), dict(family="row", launches=((12, 1, 256),))),
     _c("down_nseg4", "down", (45, 512, 512, 16, 4), dict(family="row", launches=((12, 1, 256),)))] +
    # keep bits and the f16 image of dy: the matrix-core family where segw == width
    [_c(f"covers_{w}_r{r}", "bwd", (45, w, w, r, 3), dict(family="mfma", **_COVER), keep_bits=True) for w, r in _OK3] +
    [_c(f"covers_f16dy_{w}_r{r}", "bwd_f16dy", (45, w, w, r, 3), dict(family="mfma", **_COVER), keep_bits=True) for w, r in _OK3] +
    [_c(f"covers_down_{w}_r{r}", "down", (45, w, w, r, 3), dict(family="mfma", **_COVER), keep_bits=True) for w, r in _OK3] +
    [_c("covers_not_rect", "bwd", (45, 512, 2048, 4, 1), dict(family="mfma", **_NOT)),
     _c("covers_not_rect_back", "bwd", (45, 2048, 512, 4, 1), dict(family="mfma", **_NOT)),
     _c("covers_not_192", "bwd", (45, 192, 192, 4, 3), dict(family="row", **_NOT))] +
    # every refusal, with its cause
    [_c("refuse_r65", "bwd", (45, 512, 512, 65, 3), "rank 65 unsupported at width 512"),
     _c("refuse_r65_cause", "bwd", (45, 512, 512, 65, 3), "they take ranks 1 ... 64"),
     _c("refuse_r65_down", "down", (45, 512, 512, 65, 3), "rank 65 x 3 segments unsupported at width 512"),
     _c("refuse_r32_192", "bwd", (45, 192, 192, 32, 3), "rank 32 unsupported at width 192"),
     _c("refuse_r32_192_cause", "bwd", (45, 192, 192, 32, 3), "they need width % 128 == 0"),
     _c("refuse_r3_192", "bwd", (45, 192, 192, 3, 3), "rank 3 unsupported at width 192"),
     _c("refuse_segw_64", "bwd", (45, 512, 96, 3, 1), "they need segw % 64 == 0"),
     _c("refuse_nseg2", "bwd", (45, 512, 512, 4, 2), "nseg 2 unsupported (1 or 3)"),
     _c("refuse_x_act_nseg3", "bwd", (45, 512, 512, 4, 3), "x_act needs nseg 1", x_act=True),
     _c("refuse_x_act_keep_bits", "bwd", (45, 512, 512, 4, 1), "x_act needs nseg 1, no keep bits", x_act=True, keep_bits=True),
     _c("refuse_keep_bits_192", "bwd", (45, 192, 192, 4, 3), "keep bits are read by the matrix-core kernels only", keep_bits=True),
     _c("refuse_keep_bits_192_down", "down", (45, 192, 192, 4, 3), "keep bits are recorded by the matrix-core kernels only",
        keep_bits=True),
     _c("refuse_keep_bits_rect", "bwd", (45, 512, 2048, 4, 1), "segw differs", keep_bits=True),
     _c("refuse_rect_nseg3", "bwd", (45, 512, 2048, 4, 3), "segw must equal width unless nseg is 1"),
     _c("refuse_f16dy_192", "bwd_f16dy", (45, 192, 192, 4, 3), "outside the matrix-core kernels (they need width % 128 == 0)"),
     _c("refuse_f16dy_rect", "bwd_f16dy", (45, 512, 2048, 4, 1), "outside the matrix-core kernels (segw differs from width)"),
     _c("refuse_down_wide", "down", (45, 2112, 2112, 4, 1), "width 2112 needs the matrix-core kernels: they need width % 128 == 0"),
     _c("refuse_down_4100", "down", (45, 4100, 4100, 4, 1), "width 4100 unsupported"),
     _c("refuse_down_3x32_192", "down", (45, 192, 192, 32, 3), "rank 32 x 3 segments unsupported at width 192 (64 outputs per row"),
     _c("refuse_rows_0", "bwd", (0, 512, 512, 4, 3), "rows 0")] +
    # CLIPFS_LORA_MFMA=0: the row family wherever it has an instance, nothing above r = 16, no keep bits, no f16 dy
    [_under_aid(name, shape, make, args, flags, op, "CLIPFS_LORA_MFMA=0") for name, shape, make, args, _, flags, op in _NAMED] +
    [_c("down_CLIPFS_LORA_MFMA=0", "down", (12800, 768, 768, 4, 3), dict(family="row", launches=((3200, 1, 256),)),
        env="CLIPFS_LORA_MFMA=0"),
     _c("down_r32_CLIPFS_LORA_MFMA=0", "down", (45, 512, 512, 32, 3), "switched off by CLIPFS_LORA_MFMA=0", env="CLIPFS_LORA_MFMA=0"),
     _c("keep_bits_CLIPFS_LORA_MFMA=0", "bwd", (45, 512, 512, 4, 3), "switched off by CLIPFS_LORA_MFMA=0", env="CLIPFS_LORA_MFMA=0",
        keep_bits=True)] +
    # CLIPFS_LORA_KEEP_BITS=0: the families are unchanged, keep bits are not covered
    [_c(f"{name}_CLIPFS_LORA_KEEP_BITS=0", op, shape, dict(make(*shape, *args), keep_bits_ok=0), env="CLIPFS_LORA_KEEP_BITS=0", **flags)
     for name, shape, make, args, _, flags, op in _NAMED] +
    [_c("keep_bits_CLIPFS_LORA_KEEP_BITS=0", "bwd", (45, 512, 512, 4, 3), "switched off by CLIPFS_LORA_KEEP_BITS=0",
        env="CLIPFS_LORA_KEEP_BITS=0", keep_bits=True)]
)
CASES = {c.name: c for c in TABLE}
assert len(CASES) == len(TABLE)

OK_SHAPES = [(w, w, r, n) for w in (192, 512, 768, 1024) for r in (4, 16, 17, 64) for n in (1, 3)] + [(512, 2048, 4, 1)]
BOUND_SHAPES = [c[1] for c in _NAMED]


def query(c):
    """the library's answer for row `c`: the plan as a dict, or the refusal's message"""
    from clipfs import _lib
    try:
        return _lib.lora_plan(c.op, c.rows, c.width, c.segw, c.r, c.nseg, **dict(c.flags))
    except _lib.ClipfsError as e:
        return str(e)


def matches(got, want):
    if isinstance(want, str):
        return isinstance(got, str) and want in got
    return isinstance(got, dict) and all(got[k] == v for k, v in want.items())


# ------------------------------------------------------------------ one fresh child per cached aid
AIDS = ("CLIPFS_LORA_MFMA", "CLIPFS_LORA_KEEP_BITS")


def aids():
    return sorted({c.env for c in TABLE if c.env})


def child_env(aid):
    import os
    env = {k: v for k, v in os.environ.items() if k not in AIDS}
    name, value = aid.split("=")
    env[name] = value
    return env


def child_command(call):
    """argv of a fresh interpreter that runs `call` (an expression on this module, imported as `cases`)"""
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    pkg = os.path.join(os.path.dirname(here), "jittor-clip-fewshot_amd")
    code = f"import sys; sys.path[:0] = [{here!r}, {pkg!r}]; import lora_plan_cases as cases; {call}"
    return [sys.executable, "-c", code]


def print_answers(aid):
    """child side: one JSON line with the answer to every row stated for `aid`, both _ok queries at OK_SHAPES and both
    work-size functions at BOUND_SHAPES"""
    import json
    from clipfs import _lib
    lib = _lib.load()
    print("ANSWERS " + json.dumps({"rows": {c.name: query(c) for c in TABLE if c.env == aid},
                                   "keep_bits_ok": [lib.clipfs_lora_keep_bits_ok(*s) for s in OK_SHAPES],
                                   "f16dy_ok": [lib.clipfs_lora_bwd_f16dy_ok(*s) for s in OK_SHAPES],
                                   "work_floats2": [lib.clipfs_lora_bwd_work_floats2(*s) for s in BOUND_SHAPES],
                                   "work_floats": [lib.clipfs_lora_bwd_work_floats(s[0], s[1], s[3], s[4]) for s in BOUND_SHAPES]}))
