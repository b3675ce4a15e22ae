"""Host-only: the library puts every shape of the GEMM matrix (gemm_matrix_cases.py) in the schedule class its row
claims -- tile height, split-K factor, K-steps, uneven slices -- so a retune of gemm_bm / clipfs_gemm_splits fails here,
loudly and without a GPU, instead of silently moving test_gemm_matrix_gpu.py off the code it is there to run."""
import pytest

from gemm_matrix_cases import (BK, GM, PLANE_SHAPES, SCHEDULE_CLASSES, ceil_div, lora_seg_width, plane_big_tile)


@pytest.fixture(scope="module")
def lib():
    from clipfs import _lib
    return _lib.load()


@pytest.mark.parametrize("c", SCHEDULE_CLASSES, ids=[c.name for c in SCHEDULE_CLASSES])
def test_shape_lands_in_its_schedule_class(lib, c):
    assert lib.clipfs_gemm_tile_rows(c.M, c.N) == c.tile_rows
    assert lib.clipfs_gemm_splits(c.M, c.N, c.K) == c.S
    nk = ceil_div(c.K, BK)
    assert nk == c.k_steps
    assert (nk % c.S != 0) == c.uneven
    assert (ceil_div(c.M, c.tile_rows) % GM != 0) == c.short_group
    if c.S > 1:
        assert c.K % BK == 0, "only the dense K % 32 == 0 kernels split"
        assert nk // c.S >= 1
        tiles = ceil_div(c.M, c.tile_rows) * ceil_div(c.N, 128)
        assert lib.clipfs_gemm_workspace_floats(c.M, c.N, c.K) == c.S * tiles * c.tile_rows * 128 > 0
        assert lib.clipfs_gemm_counter_ints(c.M, c.N, c.K) == tiles > 0
    else:
        assert lib.clipfs_gemm_workspace_floats(c.M, c.N, c.K) == 0
        assert lib.clipfs_gemm_counter_ints(c.M, c.N, c.K) == 0


def test_table_covers_the_classes_it_is_there_for():
    by = {(c.tile_rows, c.S) for c in SCHEDULE_CLASSES if c.K % BK == 0}
    assert {(32, 2), (64, 2), (64, 3), (32, 8), (64, 1), (32, 1)} <= by
    for rows in (32, 64):
        assert any(c.uneven and c.S == 2 and c.tile_rows == rows for c in SCHEDULE_CLASSES)
    assert any(c.S == 1 and c.tile_rows == 64 and c.short_group and c.K % BK == 0 for c in SCHEDULE_CLASSES)
    assert sum(c.K % BK != 0 for c in SCHEDULE_CLASSES) == 2
    # every row has a ragged edge, but for the per-rank shape: all of its tiles take the full-tile epilogue after the combine
    whole = [c.name for c in SCHEDULE_CLASSES if c.M % c.tile_rows == 0 and c.N % 128 == 0]
    assert whole == ["s3_tile64_per_rank"]
    assert all(c.K % 4 == 0 for c in SCHEDULE_CLASSES)  # the entry point requires it


def test_tile_rows_query_is_host_only_and_sane(lib):
    for M, N in [(1, 1), (64, 128), (12800, 768), (31031, 512), (0, 0)]:
        assert lib.clipfs_gemm_tile_rows(M, N) in (32, 64)


@pytest.mark.parametrize("s", PLANE_SHAPES, ids=[s.name for s in PLANE_SHAPES])
def test_plane_shapes(s):
    assert plane_big_tile(s.M, s.N) == s.big_tile
    assert s.K % BK == 0, "the 16-bit-plane kernels need K % 32 == 0"
    assert s.M % 128 != 0 or s.N % 128 != 0 or not s.big_tile


def test_lora_segment_widths():
    for N in sorted({c.N for c in SCHEDULE_CLASSES} | {s.N for s in PLANE_SHAPES} | {96, 200}):
        w = lora_seg_width(N)
        assert w % 32 == 0 and w % 128 != 0 and 3 * w >= N
        assert N <= 64 or 2 * w < N, f"N = {N}: the third segment would be empty"
