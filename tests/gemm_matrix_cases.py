"""The schedule classes of clipfs_gemm_nt that the GEMM matrix tests cover, in one place: test_gemm_schedule_table.py
(CPU) asserts that the built library really puts every shape in its class, test_gemm_matrix_gpu.py runs them.

A class is what the host code of csrc/gemm.hip picks from the shape: the block tile height (clipfs_gemm_tile_rows), the
split-K factor S (clipfs_gemm_splits) and the kernel (dense K % 32 == 0, or the generic K-tail kernel).  Every row keeps a
ragged M (M % tile rows != 0) or a ragged N (N % 128 != 0) unless its name says what else it is there for."""
from collections import namedtuple

BK = 32    # K-step of every GEMM kernel
GM = 8     # m-blocks per super-tile of the tile order (a launch whose m-block count is no multiple has a short last group)

# uneven: the K-steps do not divide evenly among the S slices (derived from ceil(K / 32) % S, asserted by the table test)
# short_group: ceil(M / tile rows) % GM != 0
ScheduleClass = namedtuple("ScheduleClass", "name M N K tile_rows S k_steps uneven short_group")

SCHEDULE_CLASSES = [
    ScheduleClass("s2_ragged_uneven", 995, 1003, 1056, 32, 2, 33, True, False),
    ScheduleClass("s2_tile64_uneven", 2040, 901, 288, 64, 2, 9, True, False),
    ScheduleClass("s2_fewest_steps", 1000, 480, 256, 32, 2, 8, False, False),
    ScheduleClass("s3_tile64_uneven", 1200, 1000, 800, 64, 3, 25, True, True),
    ScheduleClass("s3_tile64_per_rank", 1600, 768, 768, 64, 3, 24, False, True),
    ScheduleClass("s8_ragged_n_uneven", 250, 403, 1056, 32, 8, 33, True, False),
    ScheduleClass("unsplit_tile64_ragged", 2500, 1200, 288, 64, 1, 9, False, False),
    # 2500 rows are 40 m-blocks = five full groups; 2600 rows are 41, so the sixth group holds one m-block
    ScheduleClass("unsplit_tile64_short_group", 2600, 1200, 288, 64, 1, 9, False, True),
    ScheduleClass("unsplit_tile32_ragged", 700, 480, 128, 32, 1, 4, False, True),
    # K % 32 != 0: the generic kernel (it exists with 64-row tiles only, whatever clipfs_gemm_tile_rows answers)
    ScheduleClass("ktail_generic", 1300, 1000, 100, 64, 1, 4, False, True),
    ScheduleClass("ktail_tiny", 50, 64, 100, 32, 1, 4, False, True),
]

# 16-bit-plane kernels (csrc/gemm_bf16.hip): 64 x 128 tiles, 128 x 128 from 1024 such tiles on
PlaneShape = namedtuple("PlaneShape", "name M N K big_tile")
PLANE_SHAPES = [
    PlaneShape("small_ragged", 300, 403, 96, False),
    PlaneShape("small_1000x480", 1000, 480, 256, False),
    PlaneShape("tile128_ragged", 4100, 3970, 64, True),
]
PLANE_BIG_TILES = 1024


def ceil_div(a, b):
    return (a + b - 1) // b


def plane_big_tile(M, N):
    """gemm_bf16x3_dispatch picks the 128 x 128 tile from PLANE_BIG_TILES tiles of that size on"""
    return ceil_div(M, 128) * ceil_div(N, 128) >= PLANE_BIG_TILES


def lora_seg_width(N):
    """Width of three LoRA segments that cover N: a multiple of 32 and never of 128, so that segment boundaries fall
    inside a 128-column block tile and the last segment ends past a ragged N."""
    w = 32 * ceil_div(N, 96)
    if w % 128 == 0:
        w += 32
    assert w % 32 == 0 and w % 128 != 0 and 3 * w >= N
    return w
