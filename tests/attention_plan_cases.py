"""The case table of tests/test_attention_plan.py: what clipfs_attention_plan -- the function the exact-fp32 attention
entry points execute -- must answer, row by row.  Stated for batch 2, heads 3 (6 heads in all) unless a row says otherwise.

The LDS sizes restate the formulas the kernel files document (bytes):
  16-token tiles   two transposed images [64][16 nt + 8]; the backward adds lse, D and 16 partial-D rows of 16 nt floats
  32-token tiles   one image [64][Lp + 4] (forward, dQ pass), two and the lse / D vectors of Lp floats (dK/dV pass),
                   Lp = seq rounded up to 32 -- or the chunk length `ctok` of the long kernels
  recomputing      P^T and dS^T [seq][lp] + dS / the K, V staging buffer [seq][max(lp, 68)] + 16 floats,
                   lp = seq rounded up to 4, plus 4 when lp / 4 is even
"""
from collections import namedtuple

BATCH, HEADS = 2, 3
BH = BATCH * HEADS
LDS_LIMIT = 160 * 1024


def ceil_div(a, b):
    return -(-a // b)


def lds16(nt, backward):
    return 4 * (2 * 64 * (16 * nt + 8) + (18 * 16 * nt if backward else 0))


def lds32(tokens, images, vectors):
    lp = 32 * ceil_div(tokens, 32)
    return 4 * (images * 64 * (lp + 4) + (2 * lp if vectors else 0))


def lds_recompute(seq):
    lp = 4 * ceil_div(seq, 4)
    lp += 4 if (lp // 4) % 2 == 0 else 0
    return 4 * (2 * seq * lp + seq * max(lp, 68) + 16)


def mfma16(seq, backward, family="mfma16", bh=BH):
    nt = ceil_div(seq, 16)
    return dict(family=family, nt=nt, launches=(((2 if backward else 1) * bh, 1, 64 * nt, lds16(nt, backward)),))


def _two_pass(grid, block, tokens, backward):
    first = (grid, 1, block, lds32(tokens, 1, False))
    return (first, (grid, 1, block, lds32(tokens, 2, True))) if backward else (first,)


def mfma32(seq, backward):
    return dict(family="mfma32", launches=_two_pass(BH, 64 * min(ceil_div(seq, 32), 4), seq, backward))


def mfma_long(parts, tiles, ctok, backward):
    return dict(family="mfma_long", parts=parts, tiles=tiles, ctok=ctok,
                launches=_two_pass(BH * parts, 64 * tiles, ctok, backward))


def stream(seq, backward):
    return dict(family="stream", launches=((BH, ceil_div(seq, 4), 256, 0),) * (2 if backward else 1))


def recompute(seq, lmax):
    return dict(family="recompute", lmax=lmax, launches=((BH, 1, 256 if seq <= 64 else 512, lds_recompute(seq)),))


# plan: the dict clipfs._lib.attention_plan returns, or a substring of the refusal's message;  env: a cached aid or None
Case = namedtuple("Case", "name direction seq causal stats aligned env plan batch heads")


def _c(name, direction, seq, plan, causal=False, stats=True, aligned=True, env=None, batch=BATCH, heads=HEADS):
    return Case(name, direction, seq, causal, stats, aligned, env, plan, batch, heads)


def _both(seq, make, *args, **kw):
    """forward and backward (with the forward's out / lse / work) rows of one length"""
    tag = "_".join(f"{k}{v}" for k, v in kw.items())
    return [_c(f"{d}_{seq}{'_' + tag if tag else ''}", d, seq, make(*args, d == "bwd"), causal=seq % 2 == 1, **kw)
            for d in ("fwd", "bwd")]


# 289..1024: runs of at most 4 tiles and chunks of at most 288 tokens, both evened out over the sequence's 32-token tiles
#   289: 10 tiles -> 3 runs of 4 (4 + 4 + 2), 2 chunks of 5 tiles;   577: 19 tiles -> 5 runs of 4, 3 chunks of 7 tiles (224);
#   1024: 32 tiles -> 8 runs of 4, 4 chunks of 8 tiles
LONG_CUT = {289: (3, 4, 160), 577: (5, 4, 224), 1024: (8, 4, 256)}

TABLE = (
    [r for s in (1, 16, 17, 50, 77, 96) for r in _both(s, mfma16, s)] +
    [r for s in (97, 130, 288) for r in _both(s, mfma32, s)] +
    [r for s in (289, 577, 1024) for r in _both(s, mfma_long, *LONG_CUT[s])] +
    [r for s in (1025, 4096) for r in _both(s, stream, s)] +
    [_c("fwd_4097", "fwd", 4097, "seq 4097"), _c("bwd_4097", "bwd", 4097, "seq 4097")] +
    # a backward whose caller kept no out / lse / work: the softmax-recomputing kernel up to 96 tokens
    [_c(f"bwd_{s}_no_stats", "bwd", s, recompute(s, lmax), causal=s % 2 == 1, stats=False)
     for s, lmax in ((64, 64), (65, 80), (80, 80), (81, 96), (96, 96))] +
    [_c("bwd_97_no_stats", "bwd", 97, "needs the forward's out and lse", stats=False)] +
    # out / dqkv not 16-byte aligned: nothing on the matrix cores
    [r for s in (50, 130) for r in _both(s, stream, s, aligned=False)] +
    # live rows: causal 16-token-tile kernels or nothing (batch 3, heads 8: the text tower's shape in the GPU tests)
    [_c(f"{d}_{s}", d, s, mfma16(s, d != "fwd_packed", fam, 24), causal=True, batch=3, heads=8)
     for d, fam in (("fwd_packed", "mfma16_packed"), ("bwd_packed", "mfma16_packed"), ("bwd_packed_io", "mfma16_pinned"))
     for s in (1, 77, 96)] +
    [_c(f"{d}_97", d, 97, "no packed kernel", causal=True) for d in ("fwd_packed", "bwd_packed", "bwd_packed_io")] +
    [_c(f"{d}_77_not_causal", d, 77, "no packed kernel") for d in ("fwd_packed", "bwd_packed", "bwd_packed_io")] +
    # CLIPFS_ATTN_MFMA=0: the streaming kernels at every length (the recomputing one where there are no statistics)
    [r for s in (50, 96, 130, 577, 1025) for r in _both(s, stream, s, env="CLIPFS_ATTN_MFMA=0")] +
    [_c("bwd_80_no_stats_ATTN_MFMA=0", "bwd", 80, recompute(80, 80), stats=False, env="CLIPFS_ATTN_MFMA=0"),
     _c("bwd_packed_77_ATTN_MFMA=0", "bwd_packed", 77, "no packed kernel", causal=True, env="CLIPFS_ATTN_MFMA=0")] +
    # CLIPFS_ATTN16=0: 32-token tiles below 97 tokens as well, and no packed kernel
    [r for s in (50, 96) for r in _both(s, mfma32, s, env="CLIPFS_ATTN16=0")] +
    [r for r in _both(577, mfma_long, *LONG_CUT[577], env="CLIPFS_ATTN16=0")] +
    [_c("fwd_packed_77_ATTN16=0", "fwd_packed", 77, "no packed kernel", causal=True, env="CLIPFS_ATTN16=0")]
)
CASES = {c.name: c for c in TABLE}
assert len(CASES) == len(TABLE)

LSE_TRIPLES = ((1, 1, 1), (3, 77, 8), (2, 96, 12), (2, 97, 2), (4, 257, 16), (1, 1025, 2), (1, 4096, 1))


def query(c):
    """the library's answer for row `c`: the plan as a dict, or the refusal's message"""
    from clipfs import _lib
    try:
        return _lib.attention_plan(c.direction, c.batch, c.seq, c.heads, c.causal, stats=c.stats, aligned=c.aligned)
    except _lib.ClipfsError as e:
        return str(e)


def matches(got, want):
    return want in got if isinstance(want, str) else got == want


# ------------------------------------------------------------------ one fresh child per cached aid
AIDS = ("CLIPFS_ATTN_MFMA", "CLIPFS_ATTN16")


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
    code = f"import sys; sys.path[:0] = [{here!r}, {pkg!r}]; import attention_plan_cases as cases; {call}"
    return [sys.executable, "-c", code]


def print_answers(aid):
    """child side: one JSON line with the answer to every row stated for `aid`, clipfs_attention_bwd_packed_ok at the text
    tower's length and clipfs_attention_lse_floats of LSE_TRIPLES"""
    import json
    from clipfs import _lib
    lib = _lib.load()
    print("ANSWERS " + json.dumps({"rows": {c.name: query(c) for c in TABLE if c.env == aid},
                                   "bwd_packed_ok": lib.clipfs_attention_bwd_packed_ok(77, 1),
                                   "lse_floats": [lib.clipfs_attention_lse_floats(*t) for t in LSE_TRIPLES]}))
