"""Deep prompts (design_details["deep_prompts"]: per-block VPT_shallow of IVLP, reference jclip/model1.py:64-127) on the
host: parameter names, shapes and initialisation, the state-dict round trip, the stage-1 / stage-2 freeze rules and the
argument checks.  Models are built on the CPU (no kernel runs)."""
import os
import tempfile

import pytest
import torch


def _cfg6():
    from clipfs import synth
    return synth.ClipConfig("six", 128, 96, 6, 192, 32, 24, 1024, 128, 6)


def _sd():
    from clipfs import synth
    return synth.synth_state_dict(_cfg6(), seed=11, perturb=True)


def _build(sd, **dd):
    from jclip.model import build_model
    return build_model(sd, design_details=dd or None, device=torch.device("cpu"))


def _deep_names(model):
    return [n for n, _ in model.named_parameters() if n.endswith("VPT_shallow")]


@pytest.mark.parametrize("vd,ld", [(3, 3), (6, 2), (1, 4), (2, 1)])
def test_names_shapes_and_count(vd, ld):
    sd = _sd()
    m = _build(sd, vision_ctx=4, language_ctx=3, deep_prompts=True, vision_depth=vd, language_depth=ld)
    want = [f"transformer.resblocks.{i}.VPT_shallow" for i in range(1, ld)] + \
           [f"visual.transformer.resblocks.{i}.VPT_shallow" for i in range(1, vd)]
    got = dict(m.named_parameters())
    assert sorted(_deep_names(m)) == sorted(want)
    for n in want:
        w = 192 if n.startswith("visual.") else 128
        rows = 4 if n.startswith("visual.") else 3
        assert tuple(got[n].shape) == (rows, w)
        assert 0.005 < got[n].std().item() < 0.05  # normal(std 0.02)
    assert m.visual.transformer.resblocks[0].VPT_shallow is None and m.transformer.resblocks[0].VPT_shallow is None


def test_off_by_default():
    sd = _sd()
    assert not _deep_names(_build(sd, vision_ctx=4, vision_depth=3, language_depth=3, language_ctx=4))
    assert not _deep_names(_build(sd))
    import jclip.clip1 as C1
    assert "deep_prompts" not in C1.DESIGN_DETAILS


def test_load_vlp_default_and_override(monkeypatch):
    import jclip.clip1 as C1
    seen = []
    monkeypatch.setattr(C1, "_load", lambda name, dd, mode, device: seen.append(dd))
    C1.load_vlp("x.pkl")
    C1.load_vlp("x.pkl", design_details={"deep_prompts": True, "vision_depth": 9})
    assert seen[0] == C1.DESIGN_DETAILS
    assert seen[1] == dict(C1.DESIGN_DETAILS, deep_prompts=True, vision_depth=9)
    assert "deep_prompts" not in C1.DESIGN_DETAILS  # the default is not modified by an override


def test_state_dict_round_trip():
    from clipfs import module_io
    sd = _sd()
    dd = dict(vision_ctx=4, language_ctx=4, deep_prompts=True, vision_depth=3, language_depth=4)
    m = _build(sd, **dd)
    with torch.no_grad():
        m.visual.transformer.resblocks[2].VPT_shallow.add_(1.0)
    saved = {k: v.clone() for k, v in m.state_dict().items()}
    m2 = _build(saved, **dd)
    for k, v in m2.state_dict().items():
        assert torch.equal(v, saved[k]), k
    # Module.save / Module.load (clipfs.module_io)
    m3 = _build(sd, **dd)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "m.pkl")
        module_io.save_module(m, path)
        module_io.load_module(m3, path)
    assert torch.equal(m3.visual.transformer.resblocks[2].VPT_shallow, m.visual.transformer.resblocks[2].VPT_shallow)
    assert torch.equal(m3.transformer.resblocks[3].VPT_shallow, m.transformer.resblocks[3].VPT_shallow)


def test_freeze_rules():
    import types

    import lora_train_vlp as L
    import slow_pace as S
    m = _build(_sd(), vision_ctx=4, language_ctx=4, deep_prompts=True, vision_depth=3, language_depth=3)
    # stage 1 (lora_train_vlp.py:143-160): everything without "lora_" is frozen, the deep prompts included
    L.mark_only_lora_as_trainable(m)
    assert not any(p.requires_grad for n, p in m.named_parameters() if n.endswith("VPT_shallow"))
    # a deep prompt flagged trainable is accepted (trained, not a bias); an unknown tensor is still refused
    m.transformer.resblocks[1].VPT_shallow.requires_grad_(True)
    assert L.trainable_biases(m) == []
    assert L.trainable_deep_prompts(m) == [m.transformer.resblocks[1].VPT_shallow]
    m.ln_final.weight.requires_grad_(True)
    with pytest.raises(ValueError, match="ln_final.weight"):
        L.trainable_biases(m)
    m.ln_final.weight.requires_grad_(False)
    # stage 2 (slow_pace.py:1551-1556): every parameter whose name contains "VPT" trains
    for p in m.parameters():
        p.requires_grad_(False)
    learner = types.SimpleNamespace(ctx=torch.nn.Parameter(torch.zeros(4, 128)))
    head = S.Channel_LP(128, 3, device=torch.device("cpu"))
    tr = S.Stage2Trainer(m, learner, head, torch.zeros(2, 128), torch.zeros(3, 128))
    deep = [p for n, p in m.named_parameters() if n.endswith("VPT_shallow")]
    assert len(deep) == 4 and all(p.requires_grad for p in deep)
    assert all(any(p is q for q in tr.params) for p in deep)


def test_bad_settings_are_refused():
    sd = _sd()
    with pytest.raises(ValueError, match="vision_ctx"):
        _build(sd, vision_ctx=0, language_ctx=4, deep_prompts=True, vision_depth=3, language_depth=1)
    with pytest.raises(ValueError, match="language_ctx"):
        _build(sd, vision_ctx=4, language_ctx=0, deep_prompts=True, vision_depth=1, language_depth=3)
    with pytest.raises(ValueError, match="vision_depth"):
        _build(sd, vision_ctx=4, language_ctx=4, deep_prompts=True, vision_depth=7, language_depth=1)
    with pytest.raises(ValueError, match="language_depth"):
        _build(sd, vision_ctx=4, language_ctx=4, deep_prompts=True, vision_depth=1, language_depth=0)
    _build(sd, vision_ctx=0, deep_prompts=True, vision_depth=1, language_depth=1)  # depth 1: nothing to place


def test_tower_refuses_a_prompt_slot_without_a_prompt():
    """ABI: g_prompt without prompt, or a prompt below the floor with a slot, is CLIPFS_EINVAL before any launch."""
    import ctypes

    from clipfs import _lib
    lib = _lib.load()
    t = _lib.new_tower()
    blocks = (_lib.Block * 2)()
    t.blocks = ctypes.cast(blocks, ctypes.POINTER(_lib.Block))
    t.width, t.heads, t.layers, t.seq = 64, 1, 2, 8
    # (x and scratch are NULL: the descriptor check runs first, and a regression would stop at "null buffer")
    blocks[1].g_prompt = 16
    assert lib.clipfs_tower_fwd(ctypes.byref(t), None, 1, None, None, None) == 1
    assert b"prompt" in lib.clipfs_last_error()
    blocks[1].prompt, blocks[1].prompt_rows, blocks[1].prompt_first = 16, 0, 4
    assert lib.clipfs_tower_fwd(ctypes.byref(t), None, 1, None, None, None) == 1
    assert b"prompt" in lib.clipfs_last_error()
    blocks[0].prompt, blocks[0].g_prompt, blocks[0].prompt_rows = 16, 16, 4
    blocks[1].prompt_rows = 4
    t.grad_lo = 1
    assert lib.clipfs_tower_fwd(ctypes.byref(t), None, 1, None, None, None) == 1
    assert b"grad_lo" in lib.clipfs_last_error()
    assert [n for n, _ in _lib.Block._fields_][-4:] == ["prompt", "g_prompt", "prompt_first", "prompt_rows"]


def test_mismatched_prompt_shapes_are_refused():
    """A stored prompt or VPT whose rows do not match vision_ctx / language_ctx is a ValueError, not rows read or written
    past the tensor; the engine's descriptor checks the live tensors again (shape, slot) before any kernel sees them."""
    sd = _sd()
    dd = dict(vision_ctx=4, language_ctx=4, deep_prompts=True, vision_depth=3, language_depth=3)
    saved = {k: v.clone() for k, v in _build(sd, **dd).state_dict().items()}
    with pytest.raises(ValueError, match="transformer.resblocks.1.VPT_shallow"):
        _build(saved, **dict(dd, language_ctx=8))
    with pytest.raises(ValueError, match="VPT_shallow|visual.VPT"):
        _build(saved, **dict(dd, vision_ctx=8))
    bad = dict(saved)
    bad["visual.VPT"] = torch.zeros(2, 192)
    for k in [k for k in bad if k.startswith("visual.transformer") and k.endswith("VPT_shallow")]:
        del bad[k]
    with pytest.raises(ValueError, match="visual.VPT"):
        _build(bad, **dd)
    _build(bad, vision_ctx=4)  # shallow VPT only: loaded as before, whatever its rows
    # the live tensors: a prompt replaced by one of another shape, or a slot of another shape
    m = _build(sd, **dd)
    from clipfs.engine import Engine
    eng = Engine(m)
    eng.txt.descriptor(False, 0)
    eng.vis.descriptor(False, 0)
    blk = m.transformer.resblocks[2]
    blk.VPT_shallow = torch.nn.Parameter(torch.zeros(8, 128))
    with pytest.raises(ValueError, match="text block 2"):
        eng.txt.descriptor(False, 0)
    blk.VPT_shallow = torch.nn.Parameter(torch.zeros(4, 128))
    blk.VPT_shallow.grad_slot = torch.zeros(8, 128)
    with pytest.raises(ValueError, match="text block 2"):
        eng.txt.descriptor(False, 0)
