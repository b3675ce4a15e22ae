"""Packed (live-row) text backward of the fp16 storage mode at the C ABI: when clipfs_tower_pack_mode packs a
weight_format = 2 tower, and the argument checks of the two kernels' entry points (clipfs_attention_f16_bwd_packed,
clipfs_layernorm_bwd_rows_f16), without a GPU: every call below must return before anything is launched."""
import ctypes

import pytest

PLANES_T = ("w_qkv_t_p", "w_o_t_p", "w_fc_t_p", "w_pr_t_p")


@pytest.fixture(scope="module")
def lib():
    from clipfs import _lib
    return _lib.load()


def _tower(layers=3, width=768, seq=77, r=16, p=0.25, seed=7, causal=1, grad_lo=0, planes_from=0):
    """A cfg-5 text tower in fp16 storage mode; blocks planes_from ... carry the transposed f16 planes."""
    from clipfs import _lib
    t = _lib.new_tower()
    blocks = (_lib.Block * layers)()
    for i, b in enumerate(blocks):  # fake device addresses: the host-side checks never dereference them
        b.lora_a_qkv, b.lora_b_qkv, b.lora_mask = 4096, 8192, 7
        for j, n in enumerate(("w_qkv_p", "w_o_p", "w_fc_p", "w_pr_p")):
            setattr(b, n, 4096 * (16 + j))
        if i >= planes_from:
            for j, n in enumerate(PLANES_T):
                setattr(b, n, 4096 * (32 + j))
    t.blocks = ctypes.cast(blocks, ctypes.POINTER(_lib.Block))
    t._keep = blocks
    t.width, t.heads, t.layers, t.seq, t.causal = width, width // 64, layers, seq, causal
    t.lora_r, t.lora_scale, t.lora_dropout, t.dropout_seed = r, 0.25, p, seed
    t.weight_format, t.grad_lo = 2, grad_lo
    return t


def _mode(lib, t, batch, R):
    return lib.clipfs_tower_pack_mode(ctypes.byref(t), batch, R)


def test_fp16_tower_packs_at_the_cfg5_geometry(lib):
    # 403 captions x 77 positions, 9748 live rows, width 768, r 16, dropout 0.25
    assert _mode(lib, _tower(), 403, 9748) == 1


def test_planes_are_needed_from_the_gradient_floor_up(lib):
    # blocks below grad_lo are not walked: their planes may be missing
    assert _mode(lib, _tower(grad_lo=1, planes_from=1), 403, 9748) == 1
    assert _mode(lib, _tower(grad_lo=1, planes_from=2), 403, 9748) == 0


@pytest.mark.parametrize("plane", PLANES_T)
@pytest.mark.parametrize("block", [1, 2])
def test_one_missing_plane_falls_back(lib, plane, block):
    t = _tower(grad_lo=1)
    setattr(t.blocks[block], plane, None)
    assert _mode(lib, t, 403, 9748) == 0


def test_not_causal_falls_back(lib):
    assert _mode(lib, _tower(causal=0), 403, 9748) == 0


def test_row_count_conditions(lib):
    t = _tower()
    M = 40 * 77
    assert _mode(lib, t, 40, M // 2) == 1
    assert _mode(lib, t, 40, M // 2 + 1) == 0  # R > M / 2
    assert _mode(lib, t, 26, 26 * 30) == 0  # M = 2002 < 2048
    assert _mode(lib, t, 27, 27 * 30) == 1  # M = 2079


def test_forward_stays_dense(lib):
    t = _tower()
    assert lib.clipfs_tower_pack_fwd_mode(ctypes.byref(t), 403, 9748) == 0


def test_attention_packed_ok(lib):
    assert lib.clipfs_attention_f16_bwd_packed_ok(77, 1) == 1
    assert lib.clipfs_attention_f16_bwd_packed_ok(77, 0) == 0
    assert lib.clipfs_attention_f16_bwd_packed_ok(288, 1) == 1
    assert lib.clipfs_attention_f16_bwd_packed_ok(289, 1) == 0
    assert lib.clipfs_attention_f16_bwd_packed_ok(0, 1) == 0


def _attn(lib, seq=77, batch=4, heads=8, **null):
    names = ("qkv", "dout", "out", "lse", "dqkv", "dqkv16", "work", "off")
    p = {n: None if null.get(n, 1) is None else 4096 * (i + 1) for i, n in enumerate(names)}
    return lib.clipfs_attention_f16_bwd_packed(p["qkv"], 1, p["dout"], 1, p["out"], p["lse"], p["dqkv"], p["dqkv16"], p["work"],
                                               p["off"], batch, seq, heads, None)


@pytest.mark.parametrize("null", ["qkv", "dout", "out", "lse", "work", "off"])
def test_attention_packed_null_pointers(lib, null):
    assert _attn(lib, **{null: None}) == 1
    assert b"attention_f16_bwd_packed: null pointer" in lib.clipfs_last_error()


def test_attention_packed_needs_one_result(lib):
    assert _attn(lib, dqkv=None, dqkv16=None) == 1
    assert b"attention_f16_bwd_packed: null pointer" in lib.clipfs_last_error()


@pytest.mark.parametrize("kw", [dict(seq=289), dict(seq=0), dict(batch=0), dict(heads=0)])
def test_attention_packed_ranges(lib, kw):
    assert _attn(lib, **kw) == 1
    assert b"attention_f16_bwd_packed" in lib.clipfs_last_error()


def _ln(lib, ldx=768, lddx=768, rows=8, width=768, **null):
    names = ("dy", "x", "gamma", "mean", "rstd", "xmap", "dres", "dx", "dx16")
    p = {n: None if null.get(n, 1) is None else 4096 * (i + 1) for i, n in enumerate(names)}
    return lib.clipfs_layernorm_bwd_rows_f16(p["dy"], p["x"], ldx, p["gamma"], p["mean"], p["rstd"], p["xmap"], p["dres"],
                                             p["dx"], p["dx16"], lddx, rows, width, None)


@pytest.mark.parametrize("null", ["dy", "x", "gamma", "mean", "rstd", "xmap", "dx"])
def test_layernorm_rows_f16_null_pointers(lib, null):
    assert _ln(lib, **{null: None}) == 1
    assert b"layernorm_bwd_rows_f16: null pointer" in lib.clipfs_last_error()


@pytest.mark.parametrize("kw", [dict(ldx=256), dict(lddx=766), dict(rows=0), dict(width=770)])
def test_layernorm_rows_f16_ranges(lib, kw):
    assert _ln(lib, **kw) == 1
    assert b"layernorm_bwd_rows_f16" in lib.clipfs_last_error()
