"""Gradient floor (clipfs_tower.grad_lo) and the frozen-adapter LoRA backward at the C ABI: sizes and argument checks
only, so this runs without a GPU (every call below must return before anything is launched)."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from clipfs import _lib
    return _lib.load()


def _tower(layers=4, width=128, seq=16, r=4, p=0.25):
    from clipfs import _lib
    t = _lib.new_tower()
    blocks = (_lib.Block * layers)()
    t.blocks = ctypes.cast(blocks, ctypes.POINTER(_lib.Block))
    t._keep = blocks
    t.width, t.heads, t.layers, t.seq = width, width // 64, layers, seq
    t.lora_r, t.lora_scale, t.lora_dropout = r, 0.5, p
    return t


def test_new_tower_has_floor_zero():
    from clipfs import _lib
    t = _lib.new_tower()
    assert t.grad_lo == 0
    assert [n for n, _ in _lib.Tower._fields_][-1] == "grad_lo"  # appended at the end (ABI rule of clipfs.h)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_saved_floats_count_blocks_from_the_floor(lib, k):
    t = _tower(layers=4)
    full = lib.clipfs_tower_saved_floats(ctypes.byref(t), 3)
    assert full > 0
    t.grad_lo = k
    part = lib.clipfs_tower_saved_floats(ctypes.byref(t), 3)
    assert part * t.layers == full * (t.layers - k)


@pytest.mark.parametrize("lo", [-1, 4, 9])
def test_floor_out_of_range_is_rejected(lib, lo):
    t = _tower(layers=4)
    t.grad_lo = lo
    assert lib.clipfs_tower_saved_floats(ctypes.byref(t), 2) == 0
    assert lib.clipfs_tower_fwd(ctypes.byref(t), None, 2, None, None, None) == 1
    assert b"grad_lo" in lib.clipfs_last_error()
    assert lib.clipfs_tower_bwd(ctypes.byref(t), None, 2, None, None, 1, None) == 1
    assert b"grad_lo" in lib.clipfs_last_error()
    assert lib.clipfs_tower_bwd_sparse(ctypes.byref(t), None, None, None, 2, None, None, 1, None) == 1
    assert b"grad_lo" in lib.clipfs_last_error()


def test_floor_needs_stop_at_input(lib):
    t = _tower(layers=4)
    t.grad_lo = 2
    assert lib.clipfs_tower_bwd(ctypes.byref(t), None, 2, None, None, 0, None) == 1
    err = lib.clipfs_last_error()
    assert b"grad_lo" in err and b"stop_at_input" in err
    assert lib.clipfs_tower_bwd_sparse(ctypes.byref(t), None, None, None, 2, None, None, 0, None) == 1
    err = lib.clipfs_last_error()
    assert b"grad_lo" in err and b"stop_at_input" in err


def test_slots_below_the_floor_are_rejected(lib):
    t = _tower(layers=4)
    t.grad_lo = 2
    t.blocks[1].g_ln1_b = 256  # never dereferenced: the descriptor is refused first
    assert lib.clipfs_tower_fwd(ctypes.byref(t), None, 2, None, None, None) == 1
    assert b"below grad_lo" in lib.clipfs_last_error()


@pytest.mark.parametrize("which", ["dA", "dB"])
@pytest.mark.parametrize("fn", ["clipfs_lora_bwd", "clipfs_lora_bwd_f16dy"])
def test_lora_bwd_one_slot_null_is_rejected(lib, fn, which):
    # fake, 16-byte aligned addresses: the call must be refused before any of them is touched
    ptr = [4096 * (i + 1) for i in range(9)]
    args = dict(dy=ptr[0], x=ptr[1], t=ptr[2], A=ptr[3], B=ptr[4], dt=ptr[5], dA=ptr[6], dB=ptr[7], dx=ptr[8])
    args[which] = None
    rc = getattr(lib, fn)(args["dy"], args["x"], args["t"], args["A"], args["B"], args["dt"], args["dA"], args["dB"],
                          args["dx"], 64, 256, 256, 4, 3, 7, 0.5, 0.0, 0, 0, 0, None, 8192, None)
    assert rc == 1
    assert b"dA and dB" in lib.clipfs_last_error()
