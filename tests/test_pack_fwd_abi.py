"""Live-row text forward at the C ABI: when clipfs_tower_pack_fwd_mode packs, and the argument checks of the new entry
points, without a GPU (every call below must return before anything is launched)."""
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


def _fwd(lib, t, batch, R):
    return lib.clipfs_tower_pack_fwd_mode(ctypes.byref(t), batch, R)


def _bwd(lib, t, batch, R):
    return lib.clipfs_tower_pack_mode(ctypes.byref(t), batch, R)


def test_packs_at_the_bench_geometry(lib):
    assert _fwd(lib, _tower(), 403, 9748) == 1


@pytest.mark.parametrize("case", ["more_than_half", "fp16_storage", "bf16x3", "not_causal", "small_tower"])
def test_falls_back_with_the_backward(lib, case):
    """Wherever the backward stays dense, and outside the exact fp32 mode, the forward stays dense too."""
    t, batch, R = _tower(), 40, 200
    if case == "more_than_half":
        R = 40 * 77 // 2 + 1
    elif case == "fp16_storage":
        t.weight_format = 2
    elif case == "bf16x3":
        t.weight_format = 1
    elif case == "not_causal":
        t.causal = 0
    else:
        batch, R = 26, 26 * 30
    assert _fwd(lib, t, batch, R) == 0
    if case == "bf16x3":
        assert _bwd(lib, t, batch, R) == 1  # only the forward needs the exact K order of the fp32 kernel


@pytest.mark.parametrize("batch,R", [(27, 27 * 30), (51, 1230)])
def test_dense_split_k_keeps_the_forward_dense(lib, batch, R):
    # 2079 and 3927 rows (the latter: the per-rank share of --batch 32 --classes 51): the dense N = 512 products have too
    # few tiles and run split-K, which an unsplit R-row launch could not reproduce bitwise.  The backward still packs.
    assert lib.clipfs_gemm_splits(batch * 77, 512, 512) > 1
    assert lib.clipfs_gemm_splits(403 * 77, 512, 512) == 1
    t = _tower()
    assert _bwd(lib, t, batch, R) == 1
    assert _fwd(lib, t, batch, R) == 0


def test_dropout_the_fused_layernorm_does_not_cover(lib):
    # rank 8: the q/k/v down-projection runs on the stand-alone kernel, which draws its masks at the packed row
    assert _fwd(lib, _tower(r=8), 403, 9748) == 0
    assert _fwd(lib, _tower(r=8, p=0.0), 403, 9748) == 1
    assert _fwd(lib, _tower(r=8, seed=0), 403, 9748) == 1  # eval: no masks


def test_o_adapter_dropout_below_the_floor(lib):
    # blocks below grad_lo draw masks in the forward too
    t = _tower()
    t.blocks[0].lora_a_o, t.blocks[0].lora_b_o, t.blocks[0].lora_mask = 4096, 8192, 15
    t.grad_lo = 1
    assert _bwd(lib, t, 403, 9748) == 1
    assert _fwd(lib, t, 403, 9748) == 0
    t2 = _tower(p=0.0)
    t2.blocks[0].lora_a_o, t2.blocks[0].lora_b_o, t2.blocks[0].lora_mask = 4096, 8192, 15
    assert _fwd(lib, t2, 403, 9748) == 1


def test_rejects_bad_descriptors(lib):
    assert lib.clipfs_tower_pack_fwd_mode(None, 10, 200) == 0
    t = _tower()
    assert _fwd(lib, t, 0, 200) == 0
    t.grad_lo = 5
    assert _fwd(lib, t, 403, 9748) == 0


def _ptr(v):
    return None if v is None else 4096 * v


def _fwd_packed(lib, t, x=8, rows=16, plan=24, R=200, batch=10, saved=32, scratch=40):
    return lib.clipfs_tower_fwd_packed(ctypes.byref(t), _ptr(x), _ptr(rows), _ptr(plan), R, batch, _ptr(saved), _ptr(scratch),
                                       None)


@pytest.mark.parametrize("null", ["x", "rows", "plan", "scratch"])
def test_fwd_packed_null_buffers(lib, null):
    assert _fwd_packed(lib, _tower(), **{null: None}) == 1
    assert b"null buffer" in lib.clipfs_last_error()


@pytest.mark.parametrize("R", [-1, 0, 9, 771])
def test_fwd_packed_R_out_of_range(lib, R):
    assert _fwd_packed(lib, _tower(), R=R) == 1
    assert b"R " in lib.clipfs_last_error()


def _bwd_saved(lib, t, plan=16, R=200, batch=10, dxs=32, rows=48, dx=64, saved=80, scratch=96, stop=1):
    return lib.clipfs_tower_bwd_packed_saved(ctypes.byref(t), _ptr(dxs), _ptr(rows), _ptr(plan), R, _ptr(dx), batch,
                                             _ptr(saved), _ptr(scratch), stop, None)


@pytest.mark.parametrize("null", ["plan", "dxs", "rows", "dx", "saved", "scratch"])
def test_bwd_packed_saved_null_buffers(lib, null):
    assert _bwd_saved(lib, _tower(), **{null: None}) == 1
    assert b"null buffer" in lib.clipfs_last_error()


def test_bwd_packed_saved_needs_the_packed_forward(lib):
    # no dense fall-back: the saved tensors would be laid out for the other forward
    t = _tower()
    t.weight_format = 1
    assert _bwd_saved(lib, t, batch=40) == 1
    assert b"pack_fwd_mode 0" in lib.clipfs_last_error()
    t = _tower()
    t.grad_lo = 1
    assert _bwd_saved(lib, t, stop=0) == 1
    assert b"stop_at_input" in lib.clipfs_last_error()


def test_attention_packed_checks(lib):
    p = [4096 * (i + 1) for i in range(6)]
    assert lib.clipfs_attention_fwd_packed(p[0], p[1], p[2], None, 4, 77, 8, None) == 1
    assert b"null pointer" in lib.clipfs_last_error()
    assert lib.clipfs_attention_fwd_packed(p[0], p[1], p[2], p[3], 4, 120, 8, None) == 1
    assert b"no packed kernel" in lib.clipfs_last_error()
    assert lib.clipfs_attention_fwd_packed(p[0] + 4, p[1], p[2], p[3], 4, 77, 8, None) == 1
    assert b"misaligned" in lib.clipfs_last_error()
    assert lib.clipfs_attention_bwd_packed_io(p[0], p[1], p[2], None, p[4], p[5], 4, 77, 8, None) == 1
    assert b"null pointer" in lib.clipfs_last_error()
    assert lib.clipfs_attention_bwd_packed_io(p[0], p[1], p[2], p[3], p[4], p[5], 4, 97, 8, None) == 1
    assert b"no packed kernel" in lib.clipfs_last_error()


def test_layernorm_lora_map_checks(lib):
    p = [4096 * (i + 1) for i in range(8)]
    assert lib.clipfs_layernorm_fwd_lora_map(p[0], 512, p[1], p[2], p[3], None, None, None, 8, 512, 1e-5, p[4], p[5], 4, 3, 7,
                                             0.25, 7, 0, 0, None, None, None) == 1
    assert b"null row map" in lib.clipfs_last_error()
    # the checks of clipfs_layernorm_fwd_lora still apply
    assert lib.clipfs_layernorm_fwd_lora_map(p[0], 512, p[1], p[2], p[3], None, None, None, 8, 512, 1e-5, p[4], p[5], 32, 3, 7,
                                             0.25, 7, 0, 0, p[6], None, None) == 1
    assert b"not covered" in lib.clipfs_last_error()
