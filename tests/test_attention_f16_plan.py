"""Host-only: clipfs_attention_f16_plan -- the function clipfs_attention_f16_fwd / _bwd / _bwd_packed execute -- gives
every row of the case table (attention_f16_plan_cases.py) the kernel family, cut, launches, grid, block and dynamic LDS
the row claims.  A change of the dispatch fails here, loudly and without a GPU.  The counterpart of test_attention_plan.py
for csrc/attention_f16.hip; this family has no environment aids, so every row is asked in this process.

The rows are those of the issue that asked for the plan, derived by hand from the launchers this plan replaced
(af_threads / af_lds_bytes / af_runs) and confirmed against them: none needed a correction.  The issue leaves the LDS
sizes at 160 and 161 tokens open; they are the documented formula's (160 tokens: the 289-token chunk's sizes)."""
import ctypes as C

import pytest

import attention_f16_plan_cases as cases
from attention_f16_plan_cases import CASES, LDS_LIMIT, LONG_MAX, SHORT_MAX, TABLE, matches, query


@pytest.fixture(scope="module")
def lib():
    from clipfs import _lib
    return _lib.load()


@pytest.mark.parametrize("c", TABLE, ids=[c.name for c in TABLE])
def test_row_gets_its_plan(lib, c):
    got = query(c)
    assert matches(got, c.plan), got


def test_table_covers_what_it_is_there_for():
    plans = [c.plan for c in TABLE if not isinstance(c.plan, str)]
    assert {p["family"] for p in plans} == {"f16_short", "f16_long"}
    # the numbers of the table are the documented formula
    for tokens, (fwd, dq, dkv) in cases.LDS.items():
        assert (fwd, dq, dkv) == (cases.lds(tokens, 1, 1), cases.lds(tokens, 2, 1), cases.lds(tokens, 2, 2, True)), tokens
    assert all(l[3] <= LDS_LIMIT for p in plans for l in p["launches"]), "every dynamic LDS size fits the 160 KiB of a CU"
    assert max(l[3] for p in plans for l in p["launches"]) == 160_000
    for s in cases.SHORT_BLOCK:
        assert len(CASES[f"fwd_{s}"].plan["launches"]) == 1 and len(CASES[f"bwd_{s}"].plan["launches"]) == 2
        assert {l[0] for d in ("fwd", "bwd") for l in CASES[f"{d}_{s}"].plan["launches"]} == {cases.BH}
    for s, (parts, tiles, ctok) in cases.LONG_CUT.items():
        for d in ("fwd", "bwd"):
            assert {l[:3] for l in CASES[f"{d}_{s}"].plan["launches"]} == {(cases.BH * parts, 1, 64 * tiles)}
    # 577 tokens (ViT-L/14 at 336 px): 61 440 / 93 696 / 124 672 B
    assert [l[3] for d in ("fwd", "bwd") for l in CASES[f"{d}_577"].plan["launches"]] == [61_440, 93_696, 124_672]
    # the packed backward is the short backward of its length
    for s in (1, 77, 288):
        assert [l[2:] for l in CASES[f"bwd_packed_{s}"].plan["launches"]] == [l[2:] for l in CASES[f"bwd_{s}"].plan["launches"]]


def test_plan_for_every_length(lib):
    """For EVERY length and both masks: the forward's plan does not depend on lse (the tower runs the blocks below the
    gradient floor without statistics); the short family exactly up to 288 tokens; every LDS size within the 160 000 B
    of the largest short launch; blocks within the kernels' __launch_bounds__ (320 short forward, 576 short backward,
    512 long); no run of the long cut empty; chunks of whole tiles, at most 288 tokens."""
    from clipfs import _lib
    for causal in (False, True):
        for seq in range(1, LONG_MAX + 1):
            fwd = _lib.attention_f16_plan("fwd", 2, seq, 3, causal, stats=True)
            assert fwd == _lib.attention_f16_plan("fwd", 2, seq, 3, causal, stats=False), seq
            bwd = _lib.attention_f16_plan("bwd", 2, seq, 3, causal)
            assert len(fwd["launches"]) == 1 and len(bwd["launches"]) == 2
            for p, short_bound in ((fwd, 320), (bwd, 576)):
                assert p["family"] == ("f16_short" if seq <= SHORT_MAX else "f16_long"), seq
                assert all(l[3] <= 160_000 for l in p["launches"]), (seq, p)
                assert all(l[1] == 1 and l[2] % 64 == 0 for l in p["launches"]), (seq, p)
                if seq <= SHORT_MAX:
                    assert all(l[0] == 6 and l[2] <= short_bound for l in p["launches"]), (seq, p)
                    assert set(p) == {"family", "launches"}
                else:
                    parts, tiles, ctok = p["parts"], p["tiles"], p["ctok"]
                    assert all(l[0] == 6 * parts and l[2] == 64 * tiles <= 512 for l in p["launches"]), (seq, p)
                    assert parts * tiles * 32 >= seq > (parts - 1) * tiles * 32, (seq, p)
                    assert ctok <= SHORT_MAX and ctok % 32 == 0, (seq, p)
            if seq > SHORT_MAX:
                assert (fwd["parts"], fwd["tiles"], fwd["ctok"]) == (bwd["parts"], bwd["tiles"], bwd["ctok"])


def test_packed_ok_asks_the_plan(lib):
    """ok exactly for causal 1 <= seq <= 288"""
    from clipfs import _lib
    for seq in range(-1, 401):
        for causal in (0, 1):
            ok = lib.clipfs_attention_f16_bwd_packed_ok(seq, causal)
            assert ok == (1 if causal and 1 <= seq <= SHORT_MAX else 0), (seq, causal)
            try:
                _lib.attention_f16_plan("bwd_packed", 3, seq, 8, causal)
                planned = 1
            except _lib.ClipfsError:
                planned = 0
            assert planned == ok, (seq, causal)


def test_max_seq_is_the_plans_bound(lib):
    assert lib.clipfs_attention_f16_max_seq() == LONG_MAX


def test_query_refusals_write_nothing(lib):
    """Host-only: CLIPFS_EINVAL (1) and a message, nothing written to `plan`."""
    from clipfs import _lib
    out = _lib.AttentionPlan()
    out.launches = -7
    both = _lib.ATTN_STATS | _lib.ATTN_ALIGNED
    assert lib.clipfs_attention_f16_plan(0, 2, 77, 3, 1, both, None) == 1 and b"null plan" in lib.clipfs_last_error()
    for d in (-1, 3):
        assert lib.clipfs_attention_f16_plan(d, 2, 77, 3, 1, both, C.byref(out)) == 1
        assert f"direction {d}".encode() in lib.clipfs_last_error()
    assert lib.clipfs_attention_f16_plan(0, 0, 77, 3, 1, both, C.byref(out)) == 1
    assert lib.clipfs_attention_f16_plan(0, 2, 1025, 3, 1, both, C.byref(out)) == 1
    err = lib.clipfs_last_error()
    assert b"seq 1025" in err and b"1024" in err
    assert lib.clipfs_attention_f16_plan(2, 2, 77, 3, 1, _lib.ATTN_STATS, C.byref(out)) == 1
    assert b"misaligned pointer" in lib.clipfs_last_error()
    assert lib.clipfs_attention_f16_plan(1, 2, 77, 3, 1, _lib.ATTN_ALIGNED, C.byref(out)) == 1
    assert b"null pointer" in lib.clipfs_last_error()
    assert out.launches == -7
    assert lib.clipfs_attention_f16_plan(1, 2, 77, 3, 1, both, C.byref(out)) == 0
    assert (out.family, out.nt, out.lmax, out.launches) == (7, 0, 0, 2)
