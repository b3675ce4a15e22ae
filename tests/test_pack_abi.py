"""Packed (live-row) text backward at the C ABI: argument checks and the fall-back conditions of
clipfs_tower_pack_mode, without a GPU (every call below must return before anything is launched)."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from clipfs import _lib
    return _lib.load()


def _tower(layers=3, width=512, seq=77, r=4, p=0.25, seed=7, causal=1):
    from clipfs import _lib
    t = _lib.new_tower()
    blocks = (_lib.Block * layers)()
    for b in blocks:  # fake device addresses: the host-side checks never dereference them
        b.lora_a_qkv, b.lora_b_qkv, b.lora_mask = 4096, 8192, 7
    t.blocks = ctypes.cast(blocks, ctypes.POINTER(_lib.Block))
    t._keep = blocks
    t.width, t.heads, t.layers, t.seq, t.causal = width, width // 64, layers, seq, causal
    t.lora_r, t.lora_scale, t.lora_dropout, t.dropout_seed = r, 0.5, p, seed
    return t


def _mode(lib, t, batch, R):
    return lib.clipfs_tower_pack_mode(ctypes.byref(t), batch, R)


def test_packs_at_the_bench_geometry(lib):
    # 403 captions x 77 positions, 9748 live rows (synth_captions(403, 77, seed=1))
    assert _mode(lib, _tower(), 403, 9748) == 1


def test_more_than_half_the_rows_falls_back(lib):
    t = _tower()
    M = 40 * 77
    assert _mode(lib, t, 40, M // 2) == 1
    assert _mode(lib, t, 40, M // 2 + 1) == 0
    assert _mode(lib, t, 40, 39) == 0  # fewer rows than captions: not a plan


@pytest.mark.parametrize("case", ["not_causal", "fp16_storage", "long_seq", "o_adapter_last_block", "o_adapter_dropout",
                                  "no_keep_bits"])
def test_fallback_conditions(lib, case):
    kw = {}
    if case == "not_causal":
        kw["causal"] = 0
    elif case == "long_seq":
        kw["seq"] = 120  # no 16-token-tile kernel past 96 tokens
    elif case == "no_keep_bits":
        kw["width"] = 64  # keep bits need the matrix-core LoRA kernels (width % 128 == 0)
    t = _tower(**kw)
    if case == "fp16_storage":
        t.weight_format = 2
    elif case == "o_adapter_last_block":
        t.blocks[t.layers - 1].lora_a_o, t.blocks[t.layers - 1].lora_b_o = 4096, 8192
        t.blocks[t.layers - 1].lora_mask = 15
    elif case == "o_adapter_dropout":
        t.blocks[0].lora_a_o, t.blocks[0].lora_b_o, t.blocks[0].lora_mask = 4096, 8192, 15
    assert _mode(lib, t, 40, 200) == 0


def test_small_towers_stay_dense(lib):
    t = _tower()
    assert _mode(lib, t, 26, 26 * 30) == 0  # 2002 rows: launch-bound, nothing to gain
    assert _mode(lib, t, 27, 27 * 30) == 1  # 2079 rows


def test_o_adapter_without_dropout_packs(lib):
    t = _tower(p=0.0)
    t.blocks[0].lora_a_o, t.blocks[0].lora_b_o, t.blocks[0].lora_mask = 4096, 8192, 15
    assert _mode(lib, t, 40, 200) == 1


def test_dropout_without_seed_packs(lib):
    # eval-mode descriptor (seed 0): no masks at all, and the width has no keep-bit kernels
    assert _mode(lib, _tower(width=64, seed=0), 40, 200) == 1


def test_pack_mode_rejects_bad_descriptors(lib):
    assert lib.clipfs_tower_pack_mode(None, 10, 200) == 0
    t = _tower()
    assert _mode(lib, t, 0, 200) == 0
    t.grad_lo = 5
    assert _mode(lib, t, 40, 200) == 0


def _bwd_packed(lib, t, plan=16, R=200, batch=10, dxs=32, rows=48, dx=64, saved=80, scratch=96, stop=1):
    ptr = lambda v: None if v is None else 4096 * v  # noqa: E731
    return lib.clipfs_tower_bwd_packed(ctypes.byref(t), ptr(dxs), ptr(rows), ptr(plan), R, ptr(dx), batch, ptr(saved),
                                       ptr(scratch), stop, None)


@pytest.mark.parametrize("null", ["plan", "dxs", "rows", "dx", "saved", "scratch"])
def test_null_buffers_are_rejected(lib, null):
    assert _bwd_packed(lib, _tower(), **{null: None}) == 1
    assert b"null buffer" in lib.clipfs_last_error()


@pytest.mark.parametrize("R", [-1, 0, 9, 771])
def test_R_out_of_range_is_rejected(lib, R):
    assert _bwd_packed(lib, _tower(), R=R) == 1
    assert b"R " in lib.clipfs_last_error()


def test_floor_needs_stop_at_input(lib):
    t = _tower()
    t.grad_lo = 1
    assert _bwd_packed(lib, t, stop=0) == 1
    assert b"stop_at_input" in lib.clipfs_last_error()


def test_attention_packed_checks(lib):
    assert lib.clipfs_attention_bwd_packed_ok(77, 1) == 1
    assert lib.clipfs_attention_bwd_packed_ok(77, 0) == 0
    assert lib.clipfs_attention_bwd_packed_ok(97, 1) == 0
    p = [4096 * (i + 1) for i in range(6)]
    assert lib.clipfs_attention_bwd_packed(p[0], p[1], p[2], p[3], p[4], None, 4, 77, 8, None) == 1
    assert b"null pointer" in lib.clipfs_last_error()
    assert lib.clipfs_attention_bwd_packed(p[0], p[1], p[2], p[3], p[4], p[5], 4, 120, 8, None) == 1
    assert b"no packed kernel" in lib.clipfs_last_error()


def test_row_map_checks(lib):
    assert lib.clipfs_gather_rows_map(None, 8, 4096, 8192, 4, 8, None) == 1
    assert lib.clipfs_gather_rows_map(4096, 4, 8192, 12288, 4, 8, None) == 1  # ld < width
    assert lib.clipfs_put_rows_map(4096, None, 8192, 8, 4, 8, None) == 1
    assert b"put_rows_map" in lib.clipfs_last_error()


def test_layernorm_bwd_rows_checks(lib):
    p = [4096 * (i + 1) for i in range(8)]
    assert lib.clipfs_layernorm_bwd_rows(p[0], p[1], 512, p[2], p[3], p[4], None, None, p[5], 512, 8, 512, None) == 1
    assert b"null pointer" in lib.clipfs_last_error()
    assert lib.clipfs_layernorm_bwd_rows(p[0], p[1], 256, p[2], p[3], p[4], p[6], None, p[5], 512, 8, 512, None) == 1
    assert b"layernorm_bwd_rows" in lib.clipfs_last_error()
