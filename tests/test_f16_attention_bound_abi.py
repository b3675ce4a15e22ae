"""Which towers the fp16 storage mode keeps on the f16 MFMA attention, seen at the C ABI without a GPU: the saved record of
a block stores q | k | v as halves exactly when the tower's attention runs on those kernels (tower.hip: qkv_f16 follows
f16_attention), so clipfs_tower_saved_floats tells the two apart.  ViT-L/14 at 336 px (577 tokens) must count as the
224-px tower (257 tokens) does; past clipfs_attention_f16_max_seq() the fp32 fallback and its fp32 qkv remain."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from clipfs import _lib
    return _lib.load()


def _tower(seq, layers=2, width=1024, r=16, weight_format=2):
    from clipfs import _lib
    t = _lib.new_tower()
    blocks = (_lib.Block * layers)()
    t.blocks = ctypes.cast(blocks, ctypes.POINTER(_lib.Block))
    t._keep = blocks
    t.width, t.heads, t.layers, t.seq = width, width // 64, layers, seq
    t.lora_r, t.lora_scale, t.lora_dropout = r, 0.5, 0.0
    t.weight_format = weight_format
    return t


def _al4(n):
    return (n + 3) & ~3


def _saved_floats(t, batch, qkv_halves):
    """The fp16-format record of one block (tower.hip, saved_layout_rows; no dropout, so no keep bits) times the depth."""
    M, d, r = batch * t.seq, t.width, t.lora_r
    qkv = (M * 3 * d + 1) // 2 if qkv_halves else M * 3 * d
    slots = [M * d, 2 * M, M * d, M * 3 * r, qkv, M * d, batch * t.seq * t.heads, M * r, M * d, 2 * M, M * 2 * d]
    return sum(_al4(s) for s in slots) * t.layers


def test_max_seq_covers_vit_l14_at_336(lib):
    from clipfs import ops
    assert lib.clipfs_attention_f16_max_seq() == ops.attention_f16_max_seq() >= 577


@pytest.mark.parametrize("seq", [257, 288, 289, 577, "max"])
def test_fp16_tower_saves_qkv_as_halves_up_to_the_bound(lib, seq):
    seq = lib.clipfs_attention_f16_max_seq() if seq == "max" else seq
    t = _tower(seq)
    for batch in (1, 3):
        assert lib.clipfs_tower_saved_floats(ctypes.byref(t), batch) == _saved_floats(t, batch, qkv_halves=True)


def test_fp16_tower_past_the_bound_keeps_fp32_qkv(lib):
    t = _tower(lib.clipfs_attention_f16_max_seq() + 1)
    for batch in (1, 3):
        assert lib.clipfs_tower_saved_floats(ctypes.byref(t), batch) == _saved_floats(t, batch, qkv_halves=False)


def test_seq_past_the_bound_is_refused_on_the_host(lib):
    # fake, 16-byte aligned addresses: the call must be refused before any of them is touched
    seq = lib.clipfs_attention_f16_max_seq() + 1
    assert lib.clipfs_attention_f16_fwd(4096, 0, 8192, None, None, 1, seq, 1, 0, None) == 1
    err = lib.clipfs_last_error()
    assert f"seq {seq}".encode() in err and str(seq - 1).encode() in err
    assert lib.clipfs_attention_f16_bwd(4096, 0, 8192, 0, 12288, 16384, 20480, None, 24576, 1, seq, 1, 0, None) == 1
    err = lib.clipfs_last_error()
    assert f"seq {seq}".encode() in err and str(seq - 1).encode() in err
