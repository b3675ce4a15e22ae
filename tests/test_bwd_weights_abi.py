"""Every backward entry point of the tower refuses a descriptor whose blocks from grad_lo up lack their transposed weights
(in fp16 storage mode: the f16 planes of those as well) BEFORE anything is launched: the addresses below are fake, so a
call that got as far as a kernel would not come back with an error code.  Runs without a GPU."""
import ctypes

import pytest

T_WEIGHTS = ["w_qkv_t", "w_o_t", "w_fc_t", "w_pr_t"]
FWD_PLANES = ["w_qkv_p", "w_o_p", "w_fc_p", "w_pr_p"]


@pytest.fixture(scope="module")
def lib():
    from clipfs import _lib
    return _lib.load()


def _tower(weight_format=0, layers=3, width=512, seq=77, r=4):
    from clipfs import _lib
    t = _lib.new_tower()
    blocks = (_lib.Block * layers)()
    for i, b in enumerate(blocks):  # fake device addresses: the host-side checks never dereference them
        b.lora_a_qkv, b.lora_b_qkv, b.lora_mask = 4096, 8192, 7
        for k, n in enumerate(T_WEIGHTS):
            setattr(b, n, 4096 * (16 + 8 * i + k))
            setattr(b, n + "_p", 4096 * (80 + 8 * i + k))
        for k, n in enumerate(FWD_PLANES):
            setattr(b, n, 4096 * (160 + 8 * i + k))
    t.blocks = ctypes.cast(blocks, ctypes.POINTER(_lib.Block))
    t._keep = blocks
    t.width, t.heads, t.layers, t.seq, t.causal = width, width // 64, layers, seq, 1
    t.lora_r, t.lora_scale, t.lora_dropout, t.dropout_seed = r, 0.5, 0.25, 7
    t.weight_format = weight_format
    return t


def _p(v):
    return 4096 * v


def _call(lib, entry, t, batch=10, R=200):
    tp = ctypes.byref(t)
    if entry == "bwd":
        return lib.clipfs_tower_bwd(tp, _p(1), batch, _p(2), _p(3), 1, None)
    if entry == "bwd_sparse":
        return lib.clipfs_tower_bwd_sparse(tp, _p(4), _p(5), _p(1), batch, _p(2), _p(3), 1, None)
    fn = lib.clipfs_tower_bwd_packed if entry == "bwd_packed" else lib.clipfs_tower_bwd_packed_saved
    return fn(tp, _p(4), _p(5), _p(6), R, _p(1), batch, _p(2), _p(3), 1, None)


ENTRIES = ["bwd", "bwd_sparse", "bwd_packed"]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", T_WEIGHTS)
@pytest.mark.parametrize("block", [1, 2])
def test_fp16_storage_needs_the_transposed_f16_planes(lib, entry, name, block):
    t = _tower(weight_format=2)
    t.grad_lo = 1
    setattr(t.blocks[block], name + "_p", None)
    assert _call(lib, entry, t) == 1
    msg = lib.clipfs_last_error()
    assert b"block %d lacks f16 copies of the transposed weights" % block in msg


@pytest.mark.parametrize("weight_format", [0, 1, 2])
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", T_WEIGHTS)
def test_every_mode_needs_the_transposed_weights(lib, weight_format, entry, name):
    t = _tower(weight_format=weight_format)
    setattr(t.blocks[0], name, None)  # the LOWEST block: refused before the upper blocks' kernels are enqueued
    assert _call(lib, entry, t) == 1
    assert b"block 0 lacks transposed weights" in lib.clipfs_last_error()


@pytest.mark.parametrize("entry", ["bwd_packed", "bwd_packed_saved"])
def test_live_row_geometry_is_checked_too(lib, entry):
    # 403 captions, 9748 live rows: clipfs_tower_pack_mode / pack_fwd_mode 1, the walk would run on the packed rows
    t = _tower()
    assert lib.clipfs_tower_pack_fwd_mode(ctypes.byref(t), 403, 9748) == 1
    t.blocks[1].w_fc_t = None
    assert _call(lib, entry, t, batch=403, R=9748) == 1
    assert b"block 1 lacks transposed weights" in lib.clipfs_last_error()
