"""Host-only: clipfs_attention_plan -- the function clipfs_attention_fwd / _bwd and their packed forms execute -- gives
every row of the case table (attention_plan_cases.py) the kernel family, tile count / cut, launches, grid, block and
dynamic LDS the row claims.  A change of the dispatch fails here, loudly and without a GPU.  The counterpart of
test_gemm_f16_plan.py for csrc/attention*.hip.

The rows are those of the issue that asked for the plan; read from the code and confirmed by the query, none needed a
correction against the dispatch this plan replaced (577 tokens: 5 runs of at most 4 tiles, chunks of 224 tokens)."""
import json
import os
import subprocess

import pytest

import attention_plan_cases as cases
from attention_plan_cases import CASES, LDS_LIMIT, LSE_TRIPLES, TABLE, matches, query

IN_PROCESS = [c for c in TABLE if c.env is None]
MFMA = ("mfma16", "mfma32", "mfma_long")


@pytest.fixture(scope="module")
def lib():
    from clipfs import _lib
    return _lib.load()


@pytest.fixture(scope="module", autouse=True)
def no_aid_in_this_process():
    set_ = sorted(k for k in cases.AIDS if k in os.environ)
    assert not set_, f"the table is stated for the default dispatch; unset {set_}"


@pytest.mark.parametrize("c", IN_PROCESS, ids=[c.name for c in IN_PROCESS])
def test_row_gets_its_plan(lib, c):
    got = query(c)
    assert matches(got, c.plan), got


@pytest.mark.parametrize("aid", cases.aids())
def test_rows_under_a_cached_aid(aid):
    """The aids are read once per process: their rows are asked in one fresh child per aid.  Either aid switches the
    packed kernels off; clipfs_attention_lse_floats does not depend on them."""
    r = subprocess.run(cases.child_command(f"cases.print_answers({aid!r})"), env=cases.child_env(aid), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = json.loads([l for l in r.stdout.splitlines() if l.startswith("ANSWERS ")][-1][8:])
    want = {c.name: c.plan for c in TABLE if c.env == aid}
    assert sorted(got["rows"]) == sorted(want)
    for name, plan in want.items():
        answer = got["rows"][name]
        if isinstance(answer, dict):  # JSON has no tuples
            answer["launches"] = tuple(tuple(l) for l in answer["launches"])
        assert matches(answer, plan), (name, answer)
    assert got["bwd_packed_ok"] == 0
    assert got["lse_floats"] == [b * s * h for b, s, h in LSE_TRIPLES]
    if aid == "CLIPFS_ATTN_MFMA=0":
        assert all(isinstance(p, str) or p["family"] in ("stream", "recompute") for p in want.values())


def test_table_covers_what_it_is_there_for():
    from clipfs import _lib
    plans = [c.plan for c in TABLE if not isinstance(c.plan, str)]
    # every family clipfs_attention_plan can return: the first seven names (the last two are clipfs_attention_f16_plan's)
    assert _lib.ATTN_FAMILIES[7:] == ("f16_short", "f16_long")
    assert {p["family"] for p in plans} == set(_lib.ATTN_FAMILIES[:7])
    assert {p["nt"] for p in plans if p["family"] == "mfma16"} == {1, 2, 4, 5, 6}
    assert {p["lmax"] for p in plans if p["family"] == "recompute"} == {64, 80, 96}
    assert all(l[3] <= LDS_LIMIT for p in plans for l in p["launches"]), "every dynamic LDS size fits the 160 KiB of a CU"
    # 16-token tiles: the backward is ONE launch of two workgroups per head; the 32-token families launch twice
    for s in (1, 16, 17, 50, 77, 96):
        p = CASES[f"bwd_{s}"].plan
        assert p["nt"] == cases.ceil_div(s, 16) and len(p["launches"]) == 1 and p["launches"][0][0] == 2 * cases.BH
    for s in (97, 130, 288, 289, 577, 1024):
        assert len(CASES[f"bwd_{s}"].plan["launches"]) == 2 and len(CASES[f"fwd_{s}"].plan["launches"]) == 1
    assert [CASES[f"fwd_{s}"].plan["launches"][0][2] for s in (97, 130, 288)] == [256, 256, 256]
    assert CASES["fwd_50_envCLIPFS_ATTN16=0"].plan["launches"][0][2] == 128  # 64 * min(tiles, 4) with two tiles
    assert [CASES[f"bwd_{s}_no_stats"].plan["launches"][0][2] for s in (64, 65)] == [256, 512]
    p = CASES["fwd_577"].plan
    assert (p["parts"], p["tiles"], p["ctok"]) == (5, 4, 224) and p["launches"][0][0] == 5 * cases.BH
    assert CASES["fwd_1025"].plan["launches"] == ((cases.BH, 257, 256, 0),)


def test_forward_plan_does_not_depend_on_lse(lib):
    """For EVERY length: the forward's plan is the same with and without lse -- the tower relies on it when it runs the
    blocks below the gradient floor without statistics -- and it is an MFMA family exactly up to 1024 tokens with an
    aligned out, the streaming kernels otherwise."""
    from clipfs import _lib
    for causal in (False, True):
        for seq in range(1, 4097):
            for aligned in (True, False):
                with_ = _lib.attention_plan("fwd", 2, seq, 3, causal, stats=True, aligned=aligned)
                assert with_ == _lib.attention_plan("fwd", 2, seq, 3, causal, stats=False, aligned=aligned), seq
                assert (with_["family"] in MFMA) == (aligned and seq <= 1024), (seq, aligned, with_)
                assert all(l[3] <= LDS_LIMIT for l in with_["launches"])


def test_backward_plan_for_every_length(lib):
    """With statistics: MFMA up to 1024 aligned tokens, streaming otherwise.  Without: the recomputing kernel up to 96
    tokens whatever the alignment, a refusal above."""
    from clipfs import _lib
    for seq in range(1, 4097):
        for aligned in (True, False):
            p = _lib.attention_plan("bwd", 2, seq, 3, seq % 2 == 1, aligned=aligned)
            assert (p["family"] in MFMA) == (aligned and seq <= 1024) and (p["family"] in MFMA or p["family"] == "stream")
            assert all(l[3] <= LDS_LIMIT for l in p["launches"])
            if seq <= 96:
                assert _lib.attention_plan("bwd", 2, seq, 3, False, stats=False, aligned=aligned)["family"] == "recompute"
            else:
                with pytest.raises(_lib.ClipfsError):
                    _lib.attention_plan("bwd", 2, seq, 3, False, stats=False, aligned=aligned)


def test_packed_ok_asks_the_plan(lib):
    """ok exactly for causal seq <= 96"""
    from clipfs import _lib
    for seq in range(-1, 200):
        for causal in (0, 1):
            ok = lib.clipfs_attention_bwd_packed_ok(seq, causal)
            assert ok == (1 if causal and 1 <= seq <= 96 else 0), (seq, causal)
            if seq >= 1:
                for d in ("fwd_packed", "bwd_packed", "bwd_packed_io"):
                    try:
                        _lib.attention_plan(d, 3, seq, 8, causal)
                        planned = 1
                    except _lib.ClipfsError:
                        planned = 0
                    assert planned == ok, (d, seq, causal)


def test_lse_floats_is_one_per_query(lib):
    assert [lib.clipfs_attention_lse_floats(*t) for t in LSE_TRIPLES] == [b * s * h for b, s, h in LSE_TRIPLES]


def test_query_refusals_write_nothing(lib):
    """Host-only: CLIPFS_EINVAL (1) and a message, nothing written to `plan`."""
    import ctypes as C
    from clipfs import _lib
    out = _lib.AttentionPlan()
    out.launches = -7
    both = _lib.ATTN_STATS | _lib.ATTN_ALIGNED
    assert lib.clipfs_attention_plan(0, 2, 77, 3, 1, both, None) == 1 and b"null plan" in lib.clipfs_last_error()
    assert lib.clipfs_attention_plan(5, 2, 77, 3, 1, both, C.byref(out)) == 1 and b"direction 5" in lib.clipfs_last_error()
    assert lib.clipfs_attention_plan(0, 0, 77, 3, 1, both, C.byref(out)) == 1 and b"batch 0" in lib.clipfs_last_error()
    assert lib.clipfs_attention_plan(3, 2, 77, 3, 1, _lib.ATTN_STATS, C.byref(out)) == 1
    assert b"misaligned" in lib.clipfs_last_error()
    assert lib.clipfs_attention_plan(4, 2, 77, 3, 1, _lib.ATTN_ALIGNED, C.byref(out)) == 1
    assert b"null pointer" in lib.clipfs_last_error()
    assert out.launches == -7
    assert lib.clipfs_attention_plan(0, 2, 77, 3, 1, both, C.byref(out)) == 0 and out.launches == 1 and out.nt == 5
