"""CLIP ModifiedResNet checkpoints (RN50 family): everything that needs no GPU -- hyper-parameters from shapes, the
parameter-holding module tree and its save / load round trip, BatchNorm folding against fp64, the refusals, and the
argument checks of the three new entry points (which return before anything is launched)."""
import pickle

import pytest
import torch
import torch.nn.functional as F

import modified_resnet_ref as R

CPU = torch.device("cpu")
GEOS = R.geometries()


@pytest.fixture(scope="module", params=sorted(GEOS))
def geo_sd(request):
    geo = GEOS[request.param]
    return geo, R.synth_sd(geo), {"RN_TINY": 8, "RN_SMALL": 16}[request.param]


def test_infer_reads_the_backbone_off_the_shapes(geo_sd):
    from jclip.model import _infer
    geo, sd, heads = geo_sd
    hp = _infer(sd)
    assert hp["vision_layers"] == geo.layers and hp["vision_width"] == geo.width
    assert hp["image_resolution"] == geo.resolution and hp["embed_dim"] == geo.embed
    assert hp["vision_patch_size"] is None
    assert hp["context_length"] == geo.text.context_length and hp["transformer_layers"] == geo.text.transformer_layers
    assert hp["transformer_heads"] == geo.text.transformer_heads and hp["vocab_size"] == geo.text.vocab_size
    assert hp["vision_width"] * 32 // 64 == heads and sd["visual.attnpool.positional_embedding"].shape[1] == 64 * heads


def test_infer_rn50_key_set():
    """The published RN50: layers (3, 4, 6, 3), width 64, 224 px, 32 heads -- from an RN50-shaped key set (tensors of the
    right leading shapes are enough for ``_infer``; nothing is allocated at full size)."""
    from clipfs import resnet, synth
    from jclip.model import _infer
    sd = resnet.synth_clip_resnet_state_dict((3, 4, 6, 3), 64, 224, 1024, seed=1)
    assert len([k for k in sd if k.endswith("num_batches_tracked")]) == 3 + 3 * 16 + 4  # one per BatchNorm
    txt = synth.synth_state_dict(synth.TINY, seed=2)
    sd.update({k: v for k, v in txt.items() if not k.startswith("visual.")})
    sd["text_projection"] = torch.zeros(synth.TINY.transformer_width, 1024)
    hp = _infer(sd)
    assert hp["vision_layers"] == (3, 4, 6, 3) and hp["vision_width"] == 64 and hp["image_resolution"] == 224
    assert hp["embed_dim"] == 1024 and hp["vision_width"] * 32 // 64 == 32
    assert sd["visual.attnpool.positional_embedding"].shape == (50, 2048)


def test_build_model_holds_every_tensor_under_its_name(geo_sd, tmp_path):
    from jclip.model import ModifiedResNet, build_model
    geo, sd, heads = geo_sd
    model = build_model(sd, device=CPU)
    v = model.visual
    assert isinstance(v, ModifiedResNet) and v.VPT is None and not hasattr(v, "transformer")
    assert v.input_resolution == geo.resolution and v.output_dim == geo.embed and v.layers == geo.layers
    assert v.heads == heads and v.tokens == (geo.resolution // 32) ** 2 + 1
    assert model.dtype == torch.float32 and model.device == CPU
    own = dict(model.named_parameters())
    own.update(dict(model.named_buffers()))
    want = {k for k in sd if not k.endswith("num_batches_tracked")}
    assert set(own) == want
    assert all(not p.requires_grad for p in model.parameters())
    assert {n for n, _ in model.named_buffers()} == {k for k in want if k.endswith(("running_mean", "running_var"))}
    for k in want:
        assert torch.equal(own[k], sd[k].reshape(own[k].shape).float()), k
    # save -> load round trip (Jittor's Module.save layout: every parameter and buffer under its dotted name)
    path = str(tmp_path / "test_pkl" / "clip_model.pkl")
    model.save(path)
    other = build_model(R.synth_sd(geo, seed=99), device=CPU)
    assert not torch.equal(other.visual.bn1.running_var, v.bn1.running_var)
    other.load(path)
    got = dict(other.named_parameters())
    got.update(dict(other.named_buffers()))
    assert set(got) == want and all(torch.equal(got[k], own[k]) for k in want)


def _im2col(x, kh, stride, pad, kp):
    """[N, C, H, W] -> [N * Ho * Wo, Kp] in (ky, kx, c) column order, zero tail: the matrix clipfs_im2col_nhwc writes"""
    n, c = x.shape[:2]
    col = F.unfold(x, kh, padding=pad, stride=stride)                       # [N, C * kh * kh, L] in (c, ky, kx) order
    col = col.reshape(n, c, kh * kh, -1).permute(0, 3, 2, 1).reshape(-1, kh * kh * c)
    return torch.cat([col, torch.zeros(col.shape[0], kp - col.shape[1], dtype=col.dtype)], dim=1)


@pytest.mark.parametrize("conv,bn,stride,pad,kp", [
    ("visual.conv1", "visual.bn1", 2, 1, 28),                              # stem 3x3 / 2: K = 27, padded to 28
    ("visual.conv2", "visual.bn2", 1, 1, 9 * 8),                           # 3x3
    ("visual.layer2.0.conv1", "visual.layer2.0.bn1", 1, 0, 64),            # 1x1
    ("visual.layer2.0.downsample.0", "visual.layer2.0.downsample.1", 1, 0, 64),  # down-sample (after the mean pool)
])
def test_batchnorm_folding_fp64(conv, bn, stride, pad, kp):
    from clipfs import resnet
    sd = R.to64(R.synth_sd(GEOS["RN_TINY"]))
    w, b = resnet.fold_conv_bn(sd, conv, bn)
    cout, cin, kh, _ = sd[conv + ".weight"].shape
    assert w.dtype == torch.float64 and tuple(w.shape) == (cout, kp) and tuple(b.shape) == (cout,)
    assert (w[:, kh * kh * cin:] == 0).all()
    x = torch.randn(2, cin, 9, 7, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    want = R._bn(sd, bn, F.conv2d(x, sd[conv + ".weight"], stride=stride, padding=pad))
    got = _im2col(x, kh, stride, pad, kp) @ w.t() + b
    got = got.reshape(2, want.shape[2], want.shape[3], cout).permute(0, 3, 1, 2)
    assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()


def test_runner_folds_what_fold_conv_bn_returns():
    """The GEMM operands of the runner are the fp32 roundings of the fp64 fold (checked on the host: no launch)."""
    from clipfs import resnet
    sd = R.synth_sd(GEOS["RN_TINY"])
    c = resnet._Conv(resnet.strip_visual_prefix(sd), "conv1", "bn1", 2, 1, CPU)
    w, b = resnet.fold_conv_bn(sd, "visual.conv1", "visual.bn1")
    assert c.kp == 28 and torch.equal(c.weight, w.float()) and torch.equal(c.bias, b.float())
    assert resnet.clip_resnet_layers(resnet.strip_visual_prefix(sd)) == (1, 1, 1, 1)


def _pickle_checkpoint(sd, path):
    with open(path, "wb") as f:
        pickle.dump({k: v.numpy() for k, v in sd.items()}, f, protocol=4)
    return str(path)


def test_loader_modes(tmp_path):
    from clipfs import synth
    from jclip import clip, clip1
    from jclip.model import ModifiedResNet
    geo = GEOS["RN_TINY"]
    rn = _pickle_checkpoint(R.synth_sd(geo), tmp_path / "rn.pkl")           # carries int64 num_batches_tracked entries
    vit = _pickle_checkpoint(synth.synth_state_dict(synth.TINY, seed=3), tmp_path / "vit.pkl")
    for mode in ("res", "vit"):                                             # the backbone is read off the keys
        out = clip.load(rn, mode=mode, device=CPU)
        assert len(out) == 5 and isinstance(out[0].visual, ModifiedResNet) and out[1].n_px == geo.resolution
    with pytest.raises(NotImplementedError, match="ModifiedResNet checkpoint"):
        clip.load(vit, mode="res", device=CPU)
    with pytest.raises(RuntimeError, match="downloaded"):
        clip.load("RN50", mode="res", device=CPU)
    # visual prompts have no token sequence to join
    with pytest.raises(ValueError, match="ModifiedResNet"):
        clip1.load_vlp(rn, mode="res", device=CPU)                          # DESIGN_DETAILS: vision_ctx = 4
    with pytest.raises(ValueError, match="ModifiedResNet"):
        clip1.load_vlp(rn, device=CPU, design_details={"vision_ctx": 4})
    with pytest.raises(ValueError, match="ModifiedResNet"):
        clip1.load_vlp(rn, device=CPU, design_details={"vision_ctx": 0, "deep_prompts": True, "language_depth": 2})
    m = clip1.load_vlp(rn, device=CPU, design_details={"vision_ctx": 0, "deep_prompts": True, "vision_depth": 1,
                                                       "language_depth": 2})[0]
    assert m.transformer.resblocks[1].VPT_shallow.shape == (4, geo.text.transformer_width)
    assert isinstance(m.visual, ModifiedResNet)


def test_apply_lora_refuses_the_image_tower():
    import types
    import lora_train_vlp as L
    from jclip.model import build_model
    model = build_model(R.synth_sd(GEOS["RN_TINY"]), device=CPU)
    args = types.SimpleNamespace(encoder="vision", position="all", backbone="ViT-B/32", params=["q", "k", "v"], r=4, alpha=1,
                                 dropout_rate=0.0)
    for enc in ("vision", "both"):
        args.encoder = enc
        with pytest.raises(ValueError, match="ModifiedResNet.*encoder='text'"):
            L.apply_lora(args, model)
    # ... and 'both' adapted nothing before it refused
    assert all(b.attn.__class__.__name__ == "MultiheadAttention" for b in model.transformer.resblocks)
    assert [n for n, _ in L.towers(model)] == ["text"]


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from clipfs import _lib
    lib = _lib.load()
    p = 1 << 20  # a non-null, 16-byte aligned address: every call below returns before it would be used
    assert lib.clipfs_avgpool_nhwc(None, p, 1, 4, 4, 8, 2, None) == 1 and b"avgpool" in lib.clipfs_last_error()
    assert lib.clipfs_avgpool_nhwc(p, None, 1, 4, 4, 8, 2, None) == 1
    assert lib.clipfs_avgpool_nhwc(p + 4, p, 1, 4, 4, 8, 2, None) == 1      # misaligned
    assert lib.clipfs_avgpool_nhwc(p, p, 1, 4, 4, 6, 2, None) == 1 and b"multiple of 4" in lib.clipfs_last_error()
    assert lib.clipfs_avgpool_nhwc(p, p, 1, 4, 4, 8, 0, None) == 1 and b"k 0" in lib.clipfs_last_error()
    assert lib.clipfs_avgpool_nhwc(p, p, 1, 4, 4, 8, 5, None) == 1          # window larger than the image
    assert lib.clipfs_attnpool_tokens(None, p, p, 1, 4, 8, None) == 1 and b"attnpool_tokens" in lib.clipfs_last_error()
    assert lib.clipfs_attnpool_tokens(p, None, p, 1, 4, 8, None) == 1
    assert lib.clipfs_attnpool_tokens(p, p, None, 1, 4, 8, None) == 1
    assert lib.clipfs_attnpool_tokens(p, p, p + 8, 1, 4, 8, None) == 1
    assert lib.clipfs_attnpool_tokens(p, p, p, 1, 4, 6, None) == 1 and b"multiple of 4" in lib.clipfs_last_error()
    assert lib.clipfs_attnpool_attend(None, p, p, 1, 5, 8, None) == 1 and b"attnpool_attend" in lib.clipfs_last_error()
    assert lib.clipfs_attnpool_attend(p, None, p, 1, 5, 8, None) == 1
    assert lib.clipfs_attnpool_attend(p, p, None, 1, 5, 8, None) == 1
    assert lib.clipfs_attnpool_attend(p, p, p, 1, 1, 8, None) == 1 and b"L 1" in lib.clipfs_last_error()
    assert lib.clipfs_attnpool_attend(p, p, p, 1, 5000, 8, None) == 1
    assert lib.clipfs_attnpool_attend(p, p, p, 1, 5, 0, None) == 1 and b"heads 0" in lib.clipfs_last_error()
    assert lib.clipfs_attnpool_attend(p, p, p, 1, 5, 129, None) == 1
    assert lib.clipfs_attnpool_attend(p, p, p, 0, 5, 8, None) == 1
