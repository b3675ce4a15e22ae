"""Which biases LoRATrainer trains (lora_train_vlp.trainable_biases / FlatTrainables), on a CPU-built tiny model: the
selection follows the flags mark_only_lora_as_trainable(model, bias) sets, and a flagged parameter the fused backward
has no gradient for is refused.  No GPU needed: the flat buffer is assembled on the model's device."""
import types

import pytest
import torch


def _model(monkeypatch, params=("q", "v")):
    import lora_train_vlp as L
    from clipfs import synth
    from jclip.model import build_model
    cfg = synth.TINY
    model = build_model(synth.synth_state_dict(cfg, seed=11), device="cpu")
    monkeypatch.setitem(L.INDEX_POSITIONS_TEXT, "all", list(range(cfg.transformer_layers)))
    monkeypatch.setitem(L.INDEX_POSITIONS_VISION.setdefault("tiny", {}), "all", list(range(cfg.vision_layers)))
    args = types.SimpleNamespace(encoder="both", position="all", backbone="tiny", params=list(params), r=2, alpha=1,
                                 dropout_rate=0.0)
    layers = L.apply_lora(args, model)
    return L, cfg, model, layers


def test_selection_per_bias_mode(monkeypatch):
    L, cfg, model, layers = _model(monkeypatch)
    blocks = cfg.transformer_layers + cfg.vision_layers
    L.mark_only_lora_as_trainable(model, "none")
    assert L.trainable_biases(model) == []
    L.mark_only_lora_as_trainable(model, "all")
    names = [n for n, _ in L.trainable_biases(model)]
    assert names == [n for n, _ in model.named_parameters() if "bias" in n]
    assert len(names) == 8 * blocks + 3
    assert {"visual.ln_pre.bias", "visual.ln_post.bias", "ln_final.bias"} <= set(names)
    L.mark_only_lora_as_trainable(model, "lora_only")
    names = [n for n, _ in L.trainable_biases(model)]
    want = [f"{t}.resblocks.{i}.attn.{p}_proj.bias" for t, n in (("transformer", cfg.transformer_layers),
                                                                  ("visual.transformer", cfg.vision_layers))
            for i in range(n) for p in "qv"]
    assert sorted(names) == sorted(want)
    # the reference-faithful quirk stays in get_lora_parameters: 'lora_only' hands the optimiser no bias
    assert len(L.get_lora_parameters(model, "lora_only")) == len(L.get_lora_parameters(model, "none"))


def test_flat_buffer_holds_the_selected_biases(monkeypatch):
    L, cfg, model, layers = _model(monkeypatch)
    L.mark_only_lora_as_trainable(model, "none")
    n_none = L.FlatTrainables(model).numel
    L, cfg, model, layers = _model(monkeypatch)
    L.mark_only_lora_as_trainable(model, "lora_only")
    flat = L.FlatTrainables(model)
    assert flat.bias_offset == n_none
    assert flat.numel == n_none + 2 * sum(l.embed_dim for l in layers)
    # the flags survive the adapter re-homing, and the biases are views of the buffer with gradient slots beside them
    for l in layers:
        d = l.embed_dim
        for m in (l.q_proj, l.v_proj):
            assert m.bias.requires_grad and m.bias.grad_slot.shape == (d,)
            off = (m.bias.data_ptr() - flat.params.data_ptr()) // 4
            assert flat.bias_offset <= off < flat.numel
        assert not l.k_proj.bias.requires_grad
        # the packed bias the QKV GEMM reads is refreshed from the buffer; k is never in it
        with torch.no_grad():
            l.q_proj.bias.add_(1.0)
        flat.sync_packed()
        assert torch.equal(l.qkv_bias[:d], l.q_proj.bias) and torch.equal(l.qkv_bias[2 * d:], l.v_proj.bias)
    # state_dict returns the trained storage
    sd = L.lora_state_dict(model, "all")
    assert torch.equal(sd["transformer.resblocks.0.attn.q_proj.bias"], layers[0].q_proj.bias)


def test_all_three_qkv_biases_alias_the_packed_tensor(monkeypatch):
    L, cfg, model, layers = _model(monkeypatch, params=("q", "k", "v"))
    L.mark_only_lora_as_trainable(model, "all")
    flat = L.FlatTrainables(model)
    for l in layers:
        assert l.qkv_bias.data_ptr() == l.q_proj.bias.data_ptr()
        assert l.qkv_bias[l.embed_dim:].data_ptr() == l.k_proj.bias.data_ptr()
    assert flat._packed_dst == []


def test_flagged_parameter_without_gradient_is_refused(monkeypatch):
    L, cfg, model, layers = _model(monkeypatch)
    L.mark_only_lora_as_trainable(model, "all")
    model.visual.transformer.resblocks[0].ln_2.weight.requires_grad_(True)
    with pytest.raises(ValueError, match=r"visual\.transformer\.resblocks\.0\.ln_2\.weight"):
        L.FlatTrainables(model)
    model.visual.transformer.resblocks[0].ln_2.weight.requires_grad_(False)
    model.token_embedding.weight.requires_grad_(True)
    with pytest.raises(ValueError, match="token_embedding"):
        L.trainable_biases(model)


def test_no_warning_for_supported_modes(monkeypatch, recwarn):
    L, cfg, model, layers = _model(monkeypatch)
    L.mark_only_lora_as_trainable(model, "all")
    L.mark_only_lora_as_trainable(model, "lora_only")
    assert not [w for w in recwarn if "NOT be trained" in str(w.message)]
