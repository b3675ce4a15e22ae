"""LoRA adapters on the MLP linears (``params`` tokens ``c_fc`` / ``c_proj``) on the host: what apply_lora builds, how the
parameter filters, the flat buffer and the checkpoint see them, and the refusals -- in Python and, with fake device
addresses, in the C library before anything is launched.  Models are built on the CPU (no kernel runs)."""
import ctypes
import math
import types

import pytest
import torch

R = 4


def _args(params, r=R, p=0.25, encoder="both", position="all", backbone="small"):
    return types.SimpleNamespace(encoder=encoder, position=position, backbone=backbone, params=list(params), r=r, alpha=1,
                                 dropout_rate=p)


def _model(monkeypatch, params, text_blocks=None, vision_blocks=None, **kw):
    import lora_train_vlp as L
    from clipfs import synth
    from jclip.model import build_model
    cfg = synth.SMALL
    sd = synth.synth_state_dict(cfg, seed=11, perturb=True)
    model = build_model(sd, device=torch.device("cpu"))
    args = _args(params, **kw)
    tb = list(range(cfg.transformer_layers)) if text_blocks is None else text_blocks
    vb = list(range(cfg.vision_layers)) if vision_blocks is None else vision_blocks
    monkeypatch.setitem(L.INDEX_POSITIONS_TEXT, args.position, tb)
    monkeypatch.setitem(L.INDEX_POSITIONS_VISION.setdefault(args.backbone, {}), args.position, vb)
    return cfg, sd, model, args, L.apply_lora(args, model)


def _randomise_b(layers):
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for layer in layers:
            for tok in ("c_fc", "c_proj"):
                m = getattr(layer, tok, None)
                if m is not None:
                    m.w_lora_B.copy_(torch.randn(m.w_lora_B.shape, generator=g) * 0.05)


def test_apply_lora_structure_names_shapes_init(monkeypatch):
    import lora_train_vlp as L
    cfg, sd, model, args, layers = _model(monkeypatch, ["q", "v", "c_fc", "c_proj"])
    named = dict(model.named_parameters())
    for prefix, n, d in (("transformer", cfg.transformer_layers, cfg.transformer_width),
                         ("visual.transformer", cfg.vision_layers, cfg.vision_width)):
        for i in range(n):
            for tok, fin, fout in (("c_fc", d, 4 * d), ("c_proj", 4 * d, d)):
                a, b = named[f"{prefix}.resblocks.{i}.mlp.{tok}.w_lora_A"], named[f"{prefix}.resblocks.{i}.mlp.{tok}.w_lora_B"]
                assert tuple(a.shape) == (R, fin) and tuple(b.shape) == (fout, R)
                assert a.abs().max().item() <= 1 / math.sqrt(fin) and a.abs().max().item() > 0.5 / math.sqrt(fin)
                assert torch.count_nonzero(b) == 0
                w = named[f"{prefix}.resblocks.{i}.mlp.{tok}.weight"]
                assert torch.equal(w, sd[f"{prefix}.resblocks.{i}.mlp.{tok}.weight"]) and not w.requires_grad
                assert a.requires_grad and b.requires_grad
    blk = model.transformer.resblocks[0]
    assert isinstance(blk.mlp.c_fc, L.LinearLoRA) and isinstance(blk.mlp.c_proj, L.LinearLoRA)
    assert blk.mlp.c_fc.scaling == 1 / math.sqrt(R) and blk.mlp.c_fc.dropout_rate == 0.25
    # one name per parameter: the list entry reaches the MLP adapters without registering them twice
    assert len([n for n in named if "mlp.c_fc.w_lora_A" in n]) == cfg.transformer_layers + cfg.vision_layers
    assert layers[0].c_fc is blk.mlp.c_fc and layers[0].c_proj is blk.mlp.c_proj
    assert len(L.get_lora_parameters(model)) == (2 * 2 + 2 * 2) * len(layers)
    assert sorted(L.lora_state_dict(model)) == sorted(n for n in named if "lora_" in n)


def test_list_order_and_mlp_only_blocks(monkeypatch):
    cfg, _, model, _, layers = _model(monkeypatch, ["c_proj"], text_blocks=[1, 2], vision_blocks=[0, 2])
    tb, vb = model.transformer.resblocks, model.visual.transformer.resblocks
    assert [id(x) for x in layers] == [id(tb[1].attn), id(tb[2].attn), id(vb[0].attn), id(vb[2].attn)]
    for layer in layers:  # adapted in the MLP only: an entry all the same, with no attention adapter
        assert layer.lora_mask == 0 and layer.c_proj.is_mlp_lora and not hasattr(layer, "c_fc")
    assert not hasattr(tb[0].mlp.c_proj, "w_lora_A") and not hasattr(vb[1].mlp.c_proj, "w_lora_A")
    assert not hasattr(tb[1].mlp.c_fc, "w_lora_A")


def test_unknown_token_is_refused(monkeypatch):
    with pytest.raises(ValueError, match=r"'c_fcx' \(expected q, k, v, o, c_fc, c_proj\)"):
        _model(monkeypatch, ["q", "c_fcx"])
    with pytest.raises(ValueError, match="mlp"):
        _model(monkeypatch, ["mlp"])


@pytest.mark.parametrize("bias", ["none", "all", "lora_only"])
def test_mark_only_lora_as_trainable(monkeypatch, bias):
    import lora_train_vlp as L
    _, _, model, _, _ = _model(monkeypatch, ["q", "c_fc", "c_proj"], text_blocks=[1], vision_blocks=[0])
    L.mark_only_lora_as_trainable(model, bias)
    flags = {n: p.requires_grad for n, p in model.named_parameters()}
    assert all(v for n, v in flags.items() if "lora_" in n)
    want_bias = {"none": lambda n: False, "all": lambda n: "bias" in n,
                 "lora_only": lambda n: n in ("transformer.resblocks.1.mlp.c_fc.bias", "transformer.resblocks.1.mlp.c_proj.bias",
                                              "transformer.resblocks.1.attn.q_proj.bias",
                                              "visual.transformer.resblocks.0.mlp.c_fc.bias",
                                              "visual.transformer.resblocks.0.mlp.c_proj.bias",
                                              "visual.transformer.resblocks.0.attn.q_proj.bias")}[bias]
    for n, v in flags.items():
        if "lora_" not in n:
            assert v == want_bias(n), n
    if bias == "lora_only":
        names = [n for n, _ in L.trainable_biases(model)]
        assert "transformer.resblocks.1.mlp.c_fc.bias" in names and "visual.transformer.resblocks.0.mlp.c_proj.bias" in names


def test_flat_buffer_membership_and_views(monkeypatch):
    import lora_train_vlp as L
    cfg, _, model, _, layers = _model(monkeypatch, ["q", "c_fc", "c_proj"])
    _randomise_b(layers)
    L.mark_only_lora_as_trainable(model)
    frozen = model.visual.transformer.resblocks[1].mlp
    for m in (frozen.c_fc, frozen.c_proj):
        m.w_lora_A.requires_grad_(False)
        m.w_lora_B.requires_grad_(False)
    before = {n: p.detach().clone() for n, p in model.named_parameters() if "mlp" in n and "lora_" in n}
    flat = L.FlatTrainables(model)
    lo, hi = flat.params.data_ptr(), flat.params.data_ptr() + 4 * flat.numel
    n_in = 0
    for n, p in model.named_parameters():
        if "mlp" in n and "lora_" in n:
            assert torch.equal(p.detach(), before[n]), n  # values carried over
            inside = lo <= p.data_ptr() < hi
            assert inside == p.requires_grad, n  # frozen adapters stay out of the buffer
            if inside:
                n_in += p.numel()
                off = (p.data_ptr() - lo) // 4
                assert p.grad_slot.data_ptr() == flat.grads.data_ptr() + 4 * off and p.grad_slot.shape == p.shape
                assert p.data_ptr() % 16 == 0
    dt, dv = cfg.transformer_width, cfg.vision_width
    want = cfg.transformer_layers * 2 * R * 5 * dt + (cfg.vision_layers - 1) * 2 * R * 5 * dv
    assert n_in == want
    # the attention adapters keep their place at the head of the buffer
    assert layers[0].lora_A_qkv.data_ptr() == lo
    # a write through the buffer is a write to the parameter
    flat.params.zero_()
    assert model.transformer.resblocks[0].mlp.c_fc.w_lora_A.abs().max().item() == 0
    # one of A / B frozen alone is refused
    _, _, model2, _, _ = _model(monkeypatch, ["c_fc"])
    model2.transformer.resblocks[0].mlp.c_fc.w_lora_B.requires_grad_(False)
    with pytest.raises(ValueError, match="c_fc"):
        L.FlatTrainables(model2)


def test_save_load_round_trip_and_metadata(monkeypatch, tmp_path):
    import lora_train_vlp as L
    from clipfs import safe_pkl
    _, _, model, args, layers = _model(monkeypatch, ["q", "v", "c_fc", "c_proj"])
    _randomise_b(layers)
    path = str(tmp_path / "w" / "lora.pkl")
    L.save_lora(args, 0, layers, save_path=path)
    ck = safe_pkl.load(path)
    assert sorted(ck["weights"]["layer_0"]) == ["c_fc", "c_proj", "q_proj", "v_proj"]
    assert list(ck["metadata"]["params"]) == ["q", "v", "c_fc", "c_proj"]
    _, _, model2, _, layers2 = _model(monkeypatch, ["q", "v", "c_fc", "c_proj"])
    assert not torch.equal(layers2[0].c_proj.w_lora_B, layers[0].c_proj.w_lora_B)
    L.load_lora(args, layers2, path)
    for a, b in zip(layers, layers2):
        for tok in ("c_fc", "c_proj"):
            assert torch.equal(getattr(a, tok).w_lora_A, getattr(b, tok).w_lora_A)
            assert torch.equal(getattr(a, tok).w_lora_B, getattr(b, tok).w_lora_B)
        assert torch.equal(a.lora_A_qkv, b.lora_A_qkv)
    # the params metadata covers the new tokens
    _, _, _, args3, layers3 = _model(monkeypatch, ["q", "v", "c_fc"])
    with pytest.raises(ValueError, match="Params mismatch"):
        L.load_lora(args3, layers3, path)
    # a file written without the new tokens loads exactly as before
    _, _, _, args4, layers4 = _model(monkeypatch, ["q", "v"])
    path4 = str(tmp_path / "w" / "plain.pkl")
    L.save_lora(args4, 0, layers4, save_path=path4)
    assert sorted(safe_pkl.load(path4)["weights"]["layer_0"]) == ["q_proj", "v_proj"]
    _, _, _, _, layers5 = _model(monkeypatch, ["q", "v"])
    L.load_lora(args4, layers5, path4)
    assert torch.equal(layers4[1].lora_A_qkv, layers5[1].lora_A_qkv)


def test_fused_stage2_refuses_a_trainable_mlp_adapter(monkeypatch):
    import slow_pace as S
    _, _, model, _, _ = _model(monkeypatch, ["c_fc", "c_proj"])
    with pytest.raises(ValueError, match=r"mlp\.c_fc\.w_lora_A"):
        S.Stage2Trainer(model, None, None, None, None, fused=True)


# ---- the C library, without a device: fake addresses, the checks run before anything is enqueued ---------------------

@pytest.fixture(scope="module")
def lib():
    from clipfs import _lib
    return _lib.load()


def _tower(weight_format=0, layers=3, width=512, seq=77, r=4):
    from clipfs import _lib
    t = _lib.new_tower()
    blocks = (_lib.Block * layers)()
    for i, b in enumerate(blocks):
        for k, n in enumerate(["w_qkv_t", "w_o_t", "w_fc_t", "w_pr_t"]):
            setattr(b, n, 4096 * (16 + 8 * i + k))
            setattr(b, n + "_p", 4096 * (80 + 8 * i + k))
        for k, n in enumerate(["w_qkv_p", "w_o_p", "w_fc_p", "w_pr_p"]):
            setattr(b, n, 4096 * (160 + 8 * i + k))
    t.blocks = ctypes.cast(blocks, ctypes.POINTER(_lib.Block))
    t._keep = blocks
    t.width, t.heads, t.layers, t.seq, t.causal = width, width // 64, layers, seq, 1
    t.lora_r, t.lora_scale, t.lora_dropout, t.dropout_seed = r, 0.5, 0.25, 7
    t.weight_format = weight_format
    return t


def _adapter(b, tok):
    if tok == "c_fc":
        b.lora_a_fc, b.lora_b_fc, b.lora_mask = 4096 * 300, 4096 * 301, b.lora_mask | 16
    else:
        b.lora_a_pr, b.lora_b_pr, b.lora_mask = 4096 * 302, 4096 * 303, b.lora_mask | 32


@pytest.mark.parametrize("entry", ["fwd", "bwd"])
@pytest.mark.parametrize("tok", ["c_fc", "c_proj"])
def test_fp16_storage_refuses_mlp_adapters(lib, entry, tok):
    t = _tower(weight_format=2)
    _adapter(t.blocks[1], tok)
    tp = ctypes.byref(t)
    if entry == "fwd":
        rc = lib.clipfs_tower_fwd(tp, 4096, 10, 8192, 12288, None)
    else:
        rc = lib.clipfs_tower_bwd(tp, 4096, 10, 8192, 12288, 1, None)
    assert rc == 1
    msg = lib.clipfs_last_error().decode()
    assert "block 1" in msg and tok in msg and "fp16" in msg
    # the other modes take the same descriptor as far as the size queries
    t2 = _tower(weight_format=0)
    base = lib.clipfs_tower_saved_floats(ctypes.byref(t2), 10)
    _adapter(t2.blocks[1], tok)
    assert lib.clipfs_tower_saved_floats(ctypes.byref(t2), 10) == base + 3 * 2 * 10 * 77 * 4


@pytest.mark.parametrize("slot", ["g_lora_a_fc", "g_lora_b_fc", "g_lora_a_pr", "g_lora_b_pr"])
def test_a_slot_below_the_floor_is_refused(lib, slot):
    t = _tower()
    _adapter(t.blocks[0], "c_fc")
    _adapter(t.blocks[0], "c_proj")
    setattr(t.blocks[0], slot, 4096 * 400)
    t.grad_lo = 1
    assert lib.clipfs_tower_bwd(ctypes.byref(t), 4096, 10, 8192, 12288, 1, None) == 1
    assert b"block 0 below grad_lo 1 has gradient slots" in lib.clipfs_last_error()


def test_layouts_and_modes_move_only_with_an_mlp_adapter(lib):
    """Without an MLP adapter the saved / scratch sizes and the row / pack modes are those of a descriptor that has none
    of the new fields set; with one, the tower keeps the dense rows and the last block its full rows."""
    t = _tower()
    for b in (t.blocks[i] for i in range(3)):
        b.lora_a_qkv, b.lora_b_qkv, b.lora_mask = 4096, 8192, 7
    tp = ctypes.byref(t)
    saved, scratch = lib.clipfs_tower_saved_floats(tp, 403), lib.clipfs_tower_scratch_floats(tp, 403)
    assert lib.clipfs_tower_pack_mode(tp, 403, 9748) == 1 and lib.clipfs_tower_rows_mode(tp) == 1
    t.blocks[0].lora_a_fc = 4096 * 300  # a pointer without its mask bit is no adapter
    assert lib.clipfs_tower_saved_floats(tp, 403) == saved and lib.clipfs_tower_scratch_floats(tp, 403) == scratch
    assert lib.clipfs_tower_pack_mode(tp, 403, 9748) == 1
    _adapter(t.blocks[0], "c_proj")
    assert lib.clipfs_tower_saved_floats(tp, 403) > saved and lib.clipfs_tower_scratch_floats(tp, 403) >= scratch
    assert lib.clipfs_tower_pack_mode(tp, 403, 9748) == 0 and lib.clipfs_tower_pack_fwd_mode(tp, 403, 9748) == 0
    assert lib.clipfs_tower_rows_mode(tp) == 1  # the last block has none
    _adapter(t.blocks[2], "c_fc")
    assert lib.clipfs_tower_rows_mode(tp) == 0


def test_work_size_query(lib):
    for rows, width, r in ((300, 512, 4), (12800, 768, 16), (1600, 192, 8), (31031, 512, 64)):
        assert lib.clipfs_lora_bwd_work_floats2(rows, width, width, r, 1) == lib.clipfs_lora_bwd_work_floats(rows, width, r, 1)
        assert lib.clipfs_lora_bwd_work_floats2(rows, width, width, r, 3) == lib.clipfs_lora_bwd_work_floats(rows, width, r, 3)
    assert lib.clipfs_lora_bwd_work_floats2(300, 128, 512, 4, 1) > 0 and lib.clipfs_lora_bwd_work_floats2(300, 512, 128, 64, 1) > 0
    assert lib.clipfs_lora_bwd_work_floats2(300, 128, 512, 4, 3) == 0  # rectangular: one segment only
