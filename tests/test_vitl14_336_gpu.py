"""ViT-L/14 at 336 px (24 x 24 patches + 1 = 577 vision tokens; depth 2 + 2, LoRA r = 16) through LoRATrainer in the exact
fp32 mode and in the fp16 storage mode, against the fp64 oracle.  At 577 tokens the fp16 mode runs its attention on the
long-sequence f16 MFMA kernels (attention_f16.hip), saves qkv as halves and hands dO over as its f16 image, as it does at
257 tokens; the budgets are the ones test_fp16_precision_mode_l14 states for the 224-px tower."""
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def test_fp16_precision_mode_l14_336(dev, monkeypatch):
    """One forward_backward per mode on 3 images x 5 captions.
    Budgets: fp32 logits (100 x cosine) within 1e-4 of the oracle; fp16 logits within 5e-2, top-1 unchanged; fp16 gradient
    within 3e-2 of the fp32 gradient's largest entry, finite and non-zero; two fp16 steps with the same dropout seed are
    bitwise equal.
    The three error figures are printed before they are asserted (pytest -s); DESIGN.md section 4 is where they are kept."""
    import lora_train_vlp as L
    import test_engine_gpu as T
    from clipfs import synth
    from oracle import clip_oracle as O
    cfg = dataclasses.replace(synth.VIT_L14, image_resolution=336, vision_layers=2, transformer_layers=2, vocab_size=2048)
    assert cfg.vision_tokens == 577
    sd, model = T._build(cfg, dev, seed=17)
    args = T._args("ViT-L/14", r=16)
    lw = synth.synth_lora(cfg, 16, seed=5)
    T._apply(model, cfg, args, lw, monkeypatch)
    B, Cn = 3, 5
    img = synth.synth_images(B, 336, seed=3)
    cap = synth.synth_captions(Cn, 77, cfg.vocab_size, seed=4, max_len=20)
    tgt = synth.synth_labels(B, Cn, seed=2)
    sd64 = {k: v.double() for k, v in sd.items()}
    tl, vl = T._oracle_lora(lw, cfg)
    with torch.no_grad():
        _, wl = O.train_step_loss(sd64, img.double(), cap, tgt, tl, vl, 0.25, text_chunk=Cn)
    model.eval()
    tr = L.LoRATrainer(model)
    grads, errs, top1 = {}, {}, {}
    for mode in ("fp32", "fp16"):
        model.engine.precision = mode
        assert model.engine.precision == mode
        tr.flat.zero_grad()
        _, _, logits = tr.forward_backward(img.to(dev), cap.to(dev), tgt.to(dev))
        grads[mode] = tr.flat.grads.clone()
        errs[mode] = T._err(logits, wl)
        top1[mode] = torch.equal(logits.argmax(1).cpu(), wl.argmax(1))
    g32, g16 = grads["fp32"], grads["fp16"]
    gerr = (g16 - g32).abs().max().item() / g32.abs().max().item()
    print(f"L/14@336: fp32 logits err {errs['fp32']:.3e}, fp16 logits err {errs['fp16']:.3e}, "
          f"fp16 gradient err {gerr:.3e} of the largest fp32 entry")
    assert errs["fp32"] < 1e-4, errs["fp32"]
    assert errs["fp16"] < 5e-2, errs["fp16"]
    assert top1["fp32"] and top1["fp16"]
    assert torch.isfinite(g16).all() and g16.abs().max() > 0
    assert gerr < 3e-2, gerr


def test_fp16_step_l14_336_is_bitwise_reproducible(dev, monkeypatch):
    """Two fp16 training steps (adapter dropout 0.25) with the same dropout seed: bitwise equal logits and gradients."""
    import lora_train_vlp as L
    import test_engine_gpu as T
    from clipfs import synth
    cfg = dataclasses.replace(synth.VIT_L14, image_resolution=336, vision_layers=2, transformer_layers=2, vocab_size=2048)
    sd, model = T._build(cfg, dev, seed=17)
    args = T._args("ViT-L/14", r=16, p=0.25)
    lw = synth.synth_lora(cfg, 16, seed=5)
    T._apply(model, cfg, args, lw, monkeypatch)
    img = synth.synth_images(3, 336, seed=3).to(dev)
    cap = synth.synth_captions(5, 77, cfg.vocab_size, seed=4, max_len=20).to(dev)
    tgt = synth.synth_labels(3, 5, seed=2).to(dev)
    model.train()
    model.engine.precision = "fp16"
    tr = L.LoRATrainer(model)
    ref = None
    for _ in range(2):
        model.engine.step = 11  # the same Philox seed every time
        tr.flat.zero_grad()
        _, _, logits = tr.forward_backward(img, cap, tgt)
        got = (logits.clone(), tr.flat.grads.clone())
        if ref is None:
            ref = got
        else:
            assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    assert torch.isfinite(ref[1]).all() and ref[1].abs().max() > 0
