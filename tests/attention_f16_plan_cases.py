"""The case table of tests/test_attention_f16_plan.py: what clipfs_attention_f16_plan -- the function the fp16-storage
attention entry points execute -- must answer, row by row.  Dense rows are stated for batch 2, heads 3 (6 heads in all),
packed rows for batch 3, heads 8 (the text tower's shape in the GPU tests).

The LDS sizes (bytes) are written out as numbers; lds() restates the formula csrc/attention_f16.hip documents, and the
test checks that the two agree:
  row-major image   [Lp][72] halves (64 features + 8 pad)
  transposed image  [64][Lp + 4] halves
  Lp                the tokens in LDS rounded up to 32: seq in the short family, the chunk `ctok` in the long one
  forward           one image of each;  dQ pass: two row-major, one transposed;
  dK/dV pass        two of each and the lse / D vectors, 2 Lp floats
"""
from collections import namedtuple

BATCH, HEADS = 2, 3
BH = BATCH * HEADS
LDS_LIMIT = 160 * 1024
SHORT_MAX, LONG_MAX = 288, 1024


def ceil_div(a, b):
    return -(-a // b)


def lds(tokens, rowmajor, transposed, vectors=False):
    lp = 32 * ceil_div(tokens, 32)
    return 2 * (rowmajor * lp * 72 + transposed * 64 * (lp + 4)) + (8 * lp if vectors else 0)


# tokens in LDS -> (forward, dQ pass, dK/dV pass) bytes, as the issue that asked for the plan states them
LDS = {
    32: (9_216, 13_824, 18_688),
    96: (26_624, 40_448, 54_016),
    160: (44_032, 67_072, 89_344),
    192: (52_736, 80_384, 107_008),  # (the issue leaves 160 and 161 tokens open: these two rows are lds() alone)
    224: (61_440, 93_696, 124_672),
    256: (70_144, 107_008, 142_336),
    288: (78_848, 120_320, 160_000),
}


def _launches(grid, block, tokens, direction):
    fwd, dq, dkv = LDS[32 * ceil_div(tokens, 32)]
    return ((grid, 1, block, fwd),) if direction == "fwd" else ((grid, 1, block, dq), (grid, 1, block, dkv))


# seq -> (forward block, backward block): 64 threads per 32-token tile, at most 5 (forward) / 9 (backward) waves
SHORT_BLOCK = {1: (64, 64), 77: (192, 192), 160: (320, 320), 161: (320, 384), 257: (320, 576), 288: (320, 576)}
# seq -> (parts, tiles, ctok): runs of at most 8 tiles and chunks of at most 288 tokens, both evened out over the sequence
#   289: 10 tiles -> 2 runs of 5, 2 chunks of 5 tiles;   576: 18 tiles -> 3 runs of 6, 2 chunks of 9 tiles;
#   577: 19 tiles -> 3 runs of 7 (7 + 7 + 5), 3 chunks of 7 tiles;   1024: 32 tiles -> 4 runs of 8, 4 chunks of 8 tiles
LONG_CUT = {289: (2, 5, 160), 576: (3, 6, 288), 577: (3, 7, 224), 1024: (4, 8, 256)}


def short(seq, direction, bh=BH):
    return dict(family="f16_short", launches=_launches(bh, SHORT_BLOCK[seq][direction != "fwd"], seq, direction))


def long_(seq, direction, bh=BH):
    parts, tiles, ctok = LONG_CUT[seq]
    return dict(family="f16_long", parts=parts, tiles=tiles, ctok=ctok,
                launches=_launches(bh * parts, 64 * tiles, ctok, direction))


# plan: the dict clipfs._lib.attention_f16_plan returns, or a substring of the refusal's message
Case = namedtuple("Case", "name direction seq causal stats aligned plan batch heads")


def _c(name, direction, seq, plan, causal=False, stats=True, aligned=True, batch=BATCH, heads=HEADS):
    return Case(name, direction, seq, causal, stats, aligned, plan, batch, heads)


BIG = 32768  # BIG x BIG heads: 2^30 workgroups, one doubling short of the grid limit

TABLE = (
    [_c(f"{d}_{s}", d, s, short(s, d), causal=s % 2 == 1) for s in SHORT_BLOCK for d in ("fwd", "bwd")] +
    [_c(f"{d}_{s}", d, s, long_(s, d), causal=s % 2 == 1) for s in LONG_CUT for d in ("fwd", "bwd")] +
    # live rows over dense records: the short causal backward or nothing
    [_c(f"bwd_packed_{s}", "bwd_packed", s, short(s, "bwd", 24), causal=True, batch=3, heads=8) for s in (1, 77, 288)] +
    [_c("bwd_packed_289", "bwd_packed", 289, "no packed kernel", causal=True, batch=3, heads=8),
     _c("bwd_packed_77_not_causal", "bwd_packed", 77, "no packed kernel", batch=3, heads=8)] +
    # ranges
    [_c(f"{d}_0", d, 0, "attention_f16: seq 0 outside 1..1024") for d in ("fwd", "bwd")] +
    [_c(f"{d}_1025", d, 1025, "attention_f16: seq 1025 outside 1..1024") for d in ("fwd", "bwd")] +
    [_c("bwd_packed_0", "bwd_packed", 0, "attention_f16_bwd_packed: batch 3 seq 0 heads 8", causal=True, batch=3, heads=8)] +
    [_c(f"{d}_batch_0", d, 77, "attention_f16", causal=True, batch=0) for d in ("fwd", "bwd", "bwd_packed")] +
    [_c(f"{d}_heads_0", d, 77, "attention_f16", causal=True, heads=0) for d in ("fwd", "bwd", "bwd_packed")] +
    # this family has no fallback: a backward without out / lse / work, any call with a misaligned pointer
    [_c(f"{d}_{s}_no_stats", d, s, f"attention_f16_{d}: null pointer", causal=True, stats=False)
     for d in ("bwd", "bwd_packed") for s in (77, 288)] +
    [_c("bwd_577_no_stats", "bwd", 577, "attention_f16_bwd: null pointer", stats=False)] +
    [_c(f"{d}_{s}_misaligned", d, s, f"attention_f16_{d}: misaligned pointer", causal=True, aligned=False)
     for d in ("fwd", "bwd", "bwd_packed") for s in (77, 288)] +
    [_c(f"{d}_577_misaligned", d, 577, f"attention_f16_{d}: misaligned pointer", aligned=False) for d in ("fwd", "bwd")] +
    # batch x heads x parts must fit a grid: 2^30 heads go through as one workgroup each, not as two runs each
    [_c(f"{d}_288_big", d, 288, short(288, d, BIG * BIG), batch=BIG, heads=BIG) for d in ("fwd", "bwd")] +
    [_c(f"{d}_289_big", d, 289, "too large for seq 289", batch=BIG, heads=BIG) for d in ("fwd", "bwd")]
)
CASES = {c.name: c for c in TABLE}
assert len(CASES) == len(TABLE)


def query(c):
    """the library's answer for row `c`: the plan as a dict, or the refusal's message"""
    from clipfs import _lib
    try:
        return _lib.attention_f16_plan(c.direction, c.batch, c.seq, c.heads, c.causal, stats=c.stats, aligned=c.aligned)
    except _lib.ClipfsError as e:
        return str(e)


def matches(got, want):
    return want in got if isinstance(want, str) else got == want
