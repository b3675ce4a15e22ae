"""Host-only: clipfs_gemm_f16_plan -- the function gemm_f16_dispatch executes -- sends every row of the f16 x f16 case
table (gemm_f16_cases.py) to the kernels, row ranges and stream the row claims, for 256 compute units.  A retune of the
dispatch fails here, loudly and without a GPU, instead of silently moving test_gemm_f16_matrix_gpu.py off the kernel a
case is there to run.  The counterpart of test_gemm_schedule_table.py for csrc/gemm_f16.hip.

Where the table differs from the candidates its issue named (read from the code, corrected by the query):
  * 900 x 32768 x 128 does NOT trip the 60 % rule (3 x 128 tiles leave a remainder of 128 >= 30 % of 256, all three
    m-blocks stay): the row is 767 x 33280 x 128 (260 tiles -> one m-block of two -> 256 of 767 rows);
  * 4096 x 2048 x 64 is the 128x128 outcome of the small-problem rule; the 64x128 outcome needs < 512 tiles of 128 rows:
    3968 x 2048 x 64."""
import json
import random
import subprocess

import pytest

import gemm_f16_cases as cases
from gemm_f16_cases import CUS, EPI, KERNELS, PLAN, PLAN_TABLE, fake_pointers, gemm_args, query_plan

IN_PROCESS = [c for c in PLAN_TABLE if c.env is None]


@pytest.fixture(scope="module")
def lib():
    from clipfs import _lib
    return _lib.load()


@pytest.fixture(scope="module", autouse=True)
def no_aid_in_this_process():
    import os
    set_ = sorted(k for k in os.environ if k.startswith("CLIPFS_F16_"))
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
    got = {k: tuple(tuple(l) for l in v) for k, v in json.loads(line[6:]).items()}
    want = {c.name: c.plan for c in PLAN_TABLE if c.env == aid}
    assert got == want


def test_table_covers_what_it_is_there_for():
    launches = [l for c in PLAN_TABLE for l in c.plan]
    assert {l[0] for l in launches} == set(KERNELS), "every one of the nine kernels"
    plans = {c.name: c.plan for c in PLAN_TABLE}
    pp = ("pp_reg", "pp_lds", "ph16", "ph16_wide", "ph32")
    assert any(len(p) == 1 and p[0][0] in pp and PLAN[n].env is None for n, p in plans.items())          # no leftovers
    assert any(len(p) == 2 and p[1] == ("64x128_s2", 2048, PLAN[n].M, True) for n, p in plans.items())   # side stream
    assert plans["leftover_over_1024_tiles_4wave_on_side"][1] == ("128x128", 512, 840, True)
    assert plans["leftover_same_stream_by_aid"][1] == ("64x128", 2048, 2088, False)
    for name in ("declined_k96", "declined_seg_128odd", "declined_fill_rule", "declined_60_percent"):
        assert all(l[0] not in pp for l in plans[name]), name
    assert PLAN["declined_k96"].K < 128
    assert (cases.lora_seg_width(2560, 3, "128odd") // 128) % 2 == 1
    c = PLAN["declined_fill_rule"]
    assert (c.M // 256) * cases.ceil_div(c.N, 256) * 100 < CUS * 30
    c = PLAN["declined_60_percent"]
    assert (c.M // 256) * cases.ceil_div(c.N, 256) >= CUS and 256 * 5 < c.M * 3
    assert [plans[n][0][0] for n in ("4wave_small_64x128", "4wave_small_128x128", "4wave_256x128")] == \
        ["64x128", "128x128", "256x128"]
    assert plans["4wave_peel"] == (("256x128", 0, 8192, False), ("64x128", 8192, 8488, False))
    # register / LDS / wide on one shape
    one = [c for c in PLAN_TABLE if c.name.startswith("epi_") and (c.M, c.K) == (2088, 128)]
    assert {c.plan[0][0] for c in one if c.N == 2560} == {"pp_reg", "ph16", "ph16_wide"}
    assert {c.offset for c in one} == {None, "C", "bias", "residual"} and {c.layout for c in one} == set(cases.LAYOUTS)
    # the ping-pong kernels' row clamps: a ragged last m-block only under CLIPFS_F16_TILE=4
    assert all(l[2] % 256 == 0 for c in PLAN_TABLE if c.env is None for l in c.plan if l[0] in pp)
    assert any(l[2] % 256 for c in PLAN_TABLE if c.env == "CLIPFS_F16_TILE=4" for l in c.plan)


def test_plan_depends_on_the_cu_count(lib):
    """80 tiles pass the fill rule on 256 CUs (31 %) and miss it on 304 (26 %)"""
    c = PLAN["ph16_whole_rounds"]
    assert query_plan(c, cus=304) == (("64x128", 0, c.M, False),)
    assert query_plan(c, cus=0) in (query_plan(c, cus=256), query_plan(c, cus=304))  # 0: this device's, or 256 without one


def test_launches_partition_the_rows(lib):
    """Whatever the shape: one to three launches, in row order, covering [0, M) exactly once; only leftover rows behind a
    256 x 256 launch go to the side stream."""
    from clipfs import _lib
    rnd = random.Random(5)
    pp = ("pp_reg", "pp_lds", "ph16", "ph16_wide", "ph32")
    shapes = [(rnd.choice([1, 63, 257, 840, 2049, 2303, 8488, 20000, 65536, 200000]) + rnd.randrange(3),
               rnd.choice([8, 130, 403, 2048, 2560, 2562, 4096, 24576]), 32 * rnd.randrange(1, 40)) for _ in range(300)]
    for M, N, K in shapes:
        for epi in ("plain", "c16", "bias_res", "lora17_3seg", "lora16_3seg_128odd"):
            for cus in (64, 256, 304):
                plan = tuple(_lib.gemm_f16_plan(gemm_args(M, N, K, "tight", EPI[epi], fake_pointers()), cus))
                assert 1 <= len(plan) <= 3, (M, N, K, epi, plan)
                assert plan[0][1] == 0 and plan[-1][2] == M, (M, N, K, epi, plan)
                assert all(a[2] == b[1] for a, b in zip(plan, plan[1:])) and all(l[1] < l[2] for l in plan)
                assert all(l[0] in KERNELS for l in plan)
                if any(l[3] for l in plan):
                    assert plan[0][0] in pp and not plan[0][3] and all(l[3] for l in plan[1:]), (M, N, K, epi, plan)


def test_query_refuses_what_the_gemm_refuses(lib):
    """Host-only: CLIPFS_EINVAL (1) and a message, nothing written to `out`."""
    import ctypes as C
    from clipfs import _lib
    out = _lib.F16Plan()
    out.n = -7
    good = gemm_args(2048, 2560, 128, "tight", EPI["plain"], fake_pointers())
    assert lib.clipfs_gemm_f16_plan(None, CUS, C.byref(out)) == 1
    assert lib.clipfs_gemm_f16_plan(C.byref(good), CUS, None) == 1
    stale = gemm_args(2048, 2560, 128, "tight", EPI["plain"], fake_pointers())
    stale.struct_size -= 8
    assert lib.clipfs_gemm_f16_plan(C.byref(stale), CUS, C.byref(out)) == 1 and b"struct_size" in lib.clipfs_last_error()
    no_a16 = gemm_args(2048, 2560, 128, "tight", EPI["plain"], dict(fake_pointers(), A16=0))
    assert lib.clipfs_gemm_f16_plan(C.byref(no_a16), CUS, C.byref(out)) == 1 and b"A_f16" in lib.clipfs_last_error()
    k_tail = gemm_args(2048, 2560, 100, "tight", EPI["plain"], fake_pointers())
    k_tail.lda = k_tail.ldb = 104
    assert lib.clipfs_gemm_f16_plan(C.byref(k_tail), CUS, C.byref(out)) == 1 and b"K % 32" in lib.clipfs_last_error()
    both = gemm_args(2048, 2560, 128, "tight", EPI["alpha_lora16"], fake_pointers())
    assert lib.clipfs_gemm_f16_plan(C.byref(both), CUS, C.byref(out)) == 1
    assert b"alpha" in lib.clipfs_last_error() and b"lora_t" in lib.clipfs_last_error()
    assert out.n == -7
    assert lib.clipfs_gemm_f16_plan(C.byref(good), CUS, C.byref(out)) == 0 and out.n == 1
