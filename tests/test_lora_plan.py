"""Host-only: clipfs_lora_plan -- the function clipfs_lora_down, _bwd, _bwd_xact and _bwd_f16dy execute -- gives every row
of the case table (lora_plan_cases.py) the kernel family, matrix-core instance, slices, work layout and launches the row
claims, and every refusal its cause.  A change of the dispatch fails here, loudly and without a GPU.  The counterpart of
test_attention_plan.py for csrc/lora*.hip.

The named rows are those of the issue that asked for the plan, from a port of the rules this plan replaced; confirmed by
the query, none needed a correction, and both work-size functions return what they returned before at every row."""
import ctypes
import json
import os
import subprocess

import pytest

import lora_plan_cases as cases
from lora_plan_cases import CASES, TABLE, al4, matches, query

IN_PROCESS = [c for c in TABLE if c.env is None]


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
    assert matches(got, c.want), got
    if c.bound is not None:
        assert lib.clipfs_lora_bwd_work_floats2(c.rows, c.width, c.segw, c.r, c.nseg) == c.bound
        assert got["work_floats"] <= c.bound - 64


def _ok_default(s):
    w, segw, r, n = s
    return 1 if w % 128 == 0 and segw == w else 0


@pytest.mark.parametrize("aid", cases.aids())
def test_rows_under_a_cached_aid(lib, aid):
    """The aids are read once per process: their rows are asked in one fresh child per aid.  Neither aid changes a
    work-size function (they bound every family that may take the call)."""
    r = subprocess.run(cases.child_command(f"cases.print_answers({aid!r})"), env=cases.child_env(aid), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = json.loads([l for l in r.stdout.splitlines() if l.startswith("ANSWERS ")][-1][8:])
    want = {c.name: c.want for c in TABLE if c.env == aid}
    assert sorted(got["rows"]) == sorted(want)
    for name, plan in want.items():
        answer = got["rows"][name]
        if isinstance(answer, dict):  # JSON has no tuples
            answer["launches"] = tuple(tuple(l) for l in answer["launches"])
        assert matches(answer, plan), (name, answer)
    assert got["keep_bits_ok"] == [0] * len(cases.OK_SHAPES)
    if aid == "CLIPFS_LORA_MFMA=0":
        assert got["f16dy_ok"] == [0] * len(cases.OK_SHAPES)
        assert all(isinstance(p, str) or p["family"] == "row" for p in want.values())
        assert all(isinstance(want[f"{c.name}_{aid}"], str) == (c.r > 16 or c.op == "bwd_f16dy") for c in IN_PROCESS if c.bound)
    else:
        assert got["f16dy_ok"] == [_ok_default(s) for s in cases.OK_SHAPES]
        assert all(want[f"{c.name}_{aid}"]["family"] == c.want["family"] for c in IN_PROCESS if c.bound)
    assert got["work_floats2"] == [lib.clipfs_lora_bwd_work_floats2(*s) for s in cases.BOUND_SHAPES]
    assert got["work_floats2"] == [c.bound for c in IN_PROCESS if c.bound]
    assert got["work_floats"] == [lib.clipfs_lora_bwd_work_floats(s[0], s[1], s[3], s[4]) for s in cases.BOUND_SHAPES]


def test_ok_queries_return_the_plans_fields(lib):
    from clipfs import _lib
    for s in cases.OK_SHAPES:
        assert lib.clipfs_lora_keep_bits_ok(*s) == lib.clipfs_lora_bwd_f16dy_ok(*s) == _ok_default(s), s
        if s[0] % 128 == 0 or s[2] <= 16:  # (ranks above 16 at width 192: refused)
            p = _lib.lora_plan("bwd", 45, *s)
            assert (p["keep_bits_ok"], p["f16dy_ok"]) == (_ok_default(s),) * 2
    for s in ((512, 512, 65, 3), (512, 512, 4, 2), (512, 512, 0, 3)):  # a shape the backward refuses covers nothing
        assert lib.clipfs_lora_keep_bits_ok(*s) == lib.clipfs_lora_bwd_f16dy_ok(*s) == 0


def test_table_covers_what_it_is_there_for():
    plans = [c.want for c in IN_PROCESS if not isinstance(c.want, dict) or "groups" in c.want]
    assert {p["groups"] for p in plans if isinstance(p, dict)} == {0, 1, 2, 3, 4}
    assert {p["rq"] for p in plans if isinstance(p, dict) and "rq" in p} >= {0, 1, 4, 8, 12, 16}
    assert sum(isinstance(c.want, str) for c in IN_PROCESS) >= 10


GRID_ROWS = (1, 7, 45, 300, 1600, 9748, 12800, 31031)
GRID_WIDTHS = (64, 192, 512, 768, 1024, 3072)
GRID_RANKS = (1, 2, 3, 4, 8, 16, 17, 32, 48, 64)


def test_work_bounds_and_layout_over_a_grid(lib):
    """Both work-size functions equal the restated bound; the plan, where there is one, never writes more than they
    say, lays the dA partials out behind the dB partials at al4(slices_b nb), and has the restated slices."""
    from clipfs import _lib
    planned = 0
    for rows in GRID_ROWS:
        for width in GRID_WIDTHS:
            for nseg in (1, 3):
                for segw in (GRID_WIDTHS if nseg == 1 else (width,)):
                    for r in GRID_RANKS:
                        shape = (rows, width, segw, r, nseg)
                        ok = width % 128 == 0 and segw % 64 == 0
                        bound = cases.work_bound(*shape) if r <= 16 or segw == width or ok else 64
                        assert lib.clipfs_lora_bwd_work_floats2(*shape) == bound, shape
                        if segw == width:
                            assert lib.clipfs_lora_bwd_work_floats(rows, width, r, nseg) == bound, shape
                        try:
                            p = _lib.lora_plan("bwd", *shape)
                        except _lib.ClipfsError:
                            assert not ok and r not in (1, 2, 4, 8, 16), shape
                            continue
                        planned += 1
                        assert p["family"] == ("mfma" if ok else "row"), shape
                        assert (p["sr_b"], p["slices_b"], p["sr_a"], p["slices_a"]) == cases.slices(p["family"], *shape), shape
                        assert p["work_floats"] == cases.work_floats(p["family"], *shape) <= bound - 64, shape
                        assert p["part_a_offset"] == al4(p["slices_b"] * nseg * segw * r), shape
                        assert p["rq"] == (0 if not ok else -(-r // 4) if r <= 16 else 4 * -(-r // 16)), shape
                        frozen = _lib.lora_plan("bwd", *shape, frozen=True)
                        assert (frozen["slices_b"], frozen["slices_a"], frozen["work_floats"]) == (0, 0, 0), shape
                        assert len(frozen["launches"]) == 2 and frozen["launches"][0][0] == -(-rows // (16 if ok else 4)), shape
    assert planned > 2000


def test_query_refusals_write_nothing(lib):
    """Host-only: CLIPFS_EINVAL (1) and a message, nothing written to `plan`."""
    from clipfs import _lib
    out = _lib.LoraPlan()
    out.launches = -7
    assert lib.clipfs_lora_plan(1, 45, 512, 512, 4, 3, 0, None) == 1 and b"null plan" in lib.clipfs_last_error()
    assert lib.clipfs_lora_plan(3, 45, 512, 512, 4, 3, 0, ctypes.byref(out)) == 1 and b"operation 3" in lib.clipfs_last_error()
    assert lib.clipfs_lora_plan(1, 45, 512, 512, 65, 3, 0, ctypes.byref(out)) == 1 and b"rank 65" in lib.clipfs_last_error()
    assert out.launches == -7
    assert lib.clipfs_lora_plan(1, 45, 512, 512, 4, 3, _lib.LORA_DX, ctypes.byref(out)) == 0 and out.launches == 3


# ------------------------------------------------------------------ alignment at the ABI (fake addresses: refused before any launch)
def _bwd_args(dy):
    x, t, A, B, dt, dA, dB, dx, work = (4096 * (i + 2) for i in range(9))
    return [dy, x, t, A, B, dt, dA, dB, dx, 64, 512, 512, 4]


@pytest.mark.parametrize("fn", ["clipfs_lora_bwd", "clipfs_lora_bwd_xact", "clipfs_lora_bwd_f16dy"])
def test_misaligned_dy_is_refused(lib, fn):
    """dy 4 bytes off a 16-byte boundary: every kernel of both families reads dy 16 bytes at a time, so the call is
    refused -- it used to be sent to the row family, which reads float4s of dy all the same"""
    work = 4096 * 16
    tail = [0.5, 0.0, 0, 0, 0, 0, work, None] if fn == "clipfs_lora_bwd_xact" else [3, 7, 0.5, 0.0, 0, 0, 0, None, work, None]
    assert getattr(lib, fn)(*_bwd_args(4096 + 4), *tail) == 1
    assert b"misaligned" in lib.clipfs_last_error()
    assert getattr(lib, fn)(*_bwd_args(None), *tail) == 1  # (the aligned call would launch: only refusals are asked here)
    assert b"null pointer" in lib.clipfs_last_error()
