"""LoRA ranks above 16 at the C ABI, without a GPU: which shapes the matrix-core adapter kernels cover, that the packed
text backward keeps its keep bits and work slot at r = 32 / 64, and which ranks the tower refuses (every call below
returns before anything is launched)."""
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


@pytest.mark.parametrize("w", [512, 768, 1024])
@pytest.mark.parametrize("r", [17, 32, 64])
def test_keep_bits_cover_the_tower_widths(lib, w, r):
    assert lib.clipfs_lora_keep_bits_ok(w, w, r, 3) == 1
    assert lib.clipfs_lora_keep_bits_ok(w, w, r, 1) == 1
    assert lib.clipfs_lora_bwd_f16dy_ok(w, w, r, 3) == 1


def test_keep_bits_limits(lib):
    assert lib.clipfs_lora_keep_bits_ok(512, 512, 65, 3) == 0
    assert lib.clipfs_lora_keep_bits_ok(192, 192, 32, 3) == 0
    assert lib.clipfs_lora_keep_bits_ok(192, 192, 16, 3) == 0  # the width condition is the same at every rank
    assert lib.clipfs_lora_bwd_f16dy_ok(512, 512, 65, 3) == 0


@pytest.mark.parametrize("r", [32, 64])
def test_text_backward_packs_with_dropout(lib, r):
    # 403 captions x 77 positions, 9748 live rows: the bench's text geometry.  Needs the keep-bit slot and the adapter
    # work buffer of the packed rows to fit the dense tower's slot.
    t = _tower(r=r)
    assert lib.clipfs_tower_pack_mode(ctypes.byref(t), 403, 9748) == 1


@pytest.mark.parametrize("r", [32, 64])
def test_text_forward_rule_is_unchanged(lib, r):
    # the fused LayerNorm + down-projection covers r <= 4 only: with dropout the text forward stays dense (as at r = 8)
    assert lib.clipfs_tower_pack_fwd_mode(ctypes.byref(_tower(r=r)), 403, 9748) == 0
    assert lib.clipfs_tower_pack_fwd_mode(ctypes.byref(_tower(r=r, p=0.0)), 403, 9748) == 1


@pytest.mark.parametrize("r", [17, 32, 64])
def test_work_bound_fits_the_packed_rows(lib, r):
    # what the tower's work slot holds (sized at the dense rows) against what the packed rows need
    M, R, d = 403 * 77, 9748, 512
    assert lib.clipfs_lora_bwd_work_floats(R, d, r, 3) <= lib.clipfs_lora_bwd_work_floats(M, d, r, 3)


def test_work_bound_at_the_image_tower(lib):
    # 256 images x 50 tokens at width 768: the slice plan counts the rank groups as work, so r = 64 stays far below the
    # ~118 M floats of 32-row slices
    n = lib.clipfs_lora_bwd_work_floats(12800, 768, 64, 3)
    assert n < 40_000_000
    assert lib.clipfs_lora_bwd_work_floats(12800, 768, 16, 3) == 400 * 3 * 16 * 768 * 2 + 64  # r <= 16 unchanged


def _fwd_null(lib, t, batch=4):
    # x and scratch NULL: check_tower runs first, then the buffer check
    return lib.clipfs_tower_fwd(ctypes.byref(t), None, batch, None, None, None)


@pytest.mark.parametrize("r", [17, 32, 64])
def test_tower_accepts_ranks_up_to_64(lib, r):
    assert _fwd_null(lib, _tower(r=r)) == 1
    msg = lib.clipfs_last_error()
    assert b"null buffer" in msg and b"rank" not in msg


def test_tower_refuses_rank_65(lib):
    assert _fwd_null(lib, _tower(r=65)) == 1
    msg = lib.clipfs_last_error()
    assert b"rank 65" in msg and b"width 512" in msg


def test_tower_refuses_rank_32_at_width_192(lib):
    assert _fwd_null(lib, _tower(r=32, width=192)) == 1
    msg = lib.clipfs_last_error()
    assert b"rank 32" in msg and b"width 192" in msg
    # ranks up to 16 keep the one-wave-per-row kernels there
    assert _fwd_null(lib, _tower(r=16, width=192)) == 1
    assert b"null buffer" in lib.clipfs_last_error()


def test_lora_down_limits(lib):
    p = [4096 * (i + 1) for i in range(3)]
    # 3 x 65 outputs: past the matrix-core kernels' 192
    assert lib.clipfs_lora_down(p[0], p[1], p[2], 16, 512, 65, 3, 7, 0.0, 0, 0, 0, None, None) == 1
    assert b"rank 65" in lib.clipfs_last_error()
    # width 192 keeps the one-wave-per-row kernel's 64 outputs
    assert lib.clipfs_lora_down(p[0], p[1], p[2], 16, 192, 32, 3, 7, 0.0, 0, 0, 0, None, None) == 1
    msg = lib.clipfs_last_error()
    assert b"rank 32" in msg and b"width 192" in msg
