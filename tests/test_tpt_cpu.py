"""Host-only checks of test-time prompt tuning: the scratch size and every refusal of clipfs_tpt_objective (fake device
addresses, a NULL stream, nothing launched), select_count, the tuner's refusals on a CPU-built model, and the fp64
reference of the GPU tests against the closed-form gradient."""
import types

import pytest
import torch

from tpt_ref import tpt_closed_form, tpt_inputs, tpt_ref


@pytest.fixture(scope="module")
def lib():
    from clipfs import _lib
    return _lib.load()


@pytest.mark.parametrize("n,V,d,C", [(1, 64, 512, 403), (8, 64, 1024, 1000), (3, 5, 64, 1), (2, 1024, 64, 37)])
def test_work_floats_is_the_documented_formula(lib, n, V, d, C):
    assert lib.clipfs_tpt_work_floats(n, V, d, C) == n * (2 * V * C + C)


def test_objective_refuses_before_launching(lib):
    """Every refusal returns CLIPFS_EINVAL with the argument named; the addresses are never dereferenced."""
    feats, text, sel, loss, ent, dtext, work = (0x10000 * (i + 1) for i in range(7))

    def call(feats=feats, text=text, sel=sel, loss=loss, dtext=dtext, work=work, K=2, n=2, V=8, d=64, C=6, s=100.0, gs=1.0):
        return lib.clipfs_tpt_objective(feats, text, 0, sel, 0, K, s, gs, loss, ent, dtext, work, n, V, d, C, None)

    def refused(rc, word):
        assert rc == 1 and word in lib.clipfs_last_error(), (rc, lib.clipfs_last_error())

    refused(call(K=0), b"K 0")
    refused(call(K=9), b"K 9")
    refused(call(V=1025, K=6), b"views 1025")
    refused(call(d=1025), b"width 1025")
    refused(call(d=1028), b"width 1028")
    refused(call(d=6), b"width 6")
    refused(call(C=0), b"classes 0")
    refused(call(n=0), b"n_img 0")
    refused(call(feats=None), b"feats is NULL")
    refused(call(text=None), b"text is NULL")
    refused(call(loss=None), b"loss is NULL")
    refused(call(work=None), b"work is NULL")
    refused(call(sel=None), b"selected is NULL")
    refused(call(feats=feats + 4), b"16-byte")
    refused(call(dtext=dtext + 8), b"16-byte")
    refused(call(s=float("inf")), b"logit_scale")
    refused(call(gs=float("nan")), b"grad_scale")


def test_select_count():
    from tpt import select_count
    assert (select_count(64, 0.1), select_count(5, 0.1), select_count(64, 1.0)) == (6, 1, 64)
    assert (select_count(1024, 0.1), select_count(513, 0.1), select_count(1, 0.5)) == (102, 51, 1)


def _cpu_model():
    from clipfs import synth
    from jclip.model import build_model
    cfg = synth.TINY
    model = build_model(synth.synth_state_dict(cfg, seed=11), device=torch.device("cpu"))
    ids = synth.synth_captions(3, cfg.context_length, cfg.vocab_size, seed=4, max_len=10)
    learner = types.SimpleNamespace(ctx=torch.nn.Parameter(model.token_embedding.weight.data[ids[0, 1:5]].clone()),
                                    tokenized_prompts=ids)
    return cfg, model, learner


def test_tuner_refusals(monkeypatch):
    import lora_train_vlp as L
    from tpt import TestTimePromptTuner
    cfg, model, learner = _cpu_model()
    TestTimePromptTuner(model, learner, rho=1.0, steps=3, loss_scale=4096.0)  # a frozen model is accepted
    for rho in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="rho"):
            TestTimePromptTuner(model, learner, rho=rho)
    for steps in (0, -1, 1.5):
        with pytest.raises(ValueError, match="steps"):
            TestTimePromptTuner(model, learner, steps=steps)
    for scale in (0.0, -2.0, float("inf"), "dynamic"):
        with pytest.raises(ValueError, match="loss_scale"):
            TestTimePromptTuner(model, learner, loss_scale=scale)
    tuner = TestTimePromptTuner(model, learner)
    with pytest.raises(ValueError, match="1025 views"):
        tuner.adapt_features(torch.zeros(1, 1025, cfg.embed_dim))
    with pytest.raises(ValueError, match="1025 views"):
        tuner.adapt_views(torch.zeros(1, 1025, 3, 2, 2))
    # a trainable bias, then trainable adapters: named, with the remedy
    model.ln_final.bias.requires_grad_(True)
    with pytest.raises(ValueError, match=r"ln_final\.bias.*requires_grad_\(False\)"):
        TestTimePromptTuner(model, learner)
    with pytest.raises(ValueError, match=r"requires_grad_\(False\)"):
        tuner.adapt_features(torch.zeros(1, 8, cfg.embed_dim))  # ... and a flag set after construction is seen too
    model.ln_final.bias.requires_grad_(False)
    args = types.SimpleNamespace(encoder="both", position="all", backbone="tiny", params=["q", "k", "v"], r=4, alpha=1,
                                 dropout_rate=0.0)
    monkeypatch.setitem(L.INDEX_POSITIONS_TEXT, "all", list(range(cfg.transformer_layers)))
    monkeypatch.setitem(L.INDEX_POSITIONS_VISION.setdefault("tiny", {}), "all", list(range(cfg.vision_layers)))
    L.apply_lora(args, model)
    with pytest.raises(ValueError, match=r"transformer\.resblocks\.0\..*lora.*requires_grad_\(False\)"):
        TestTimePromptTuner(model, learner)
    for n, p in model.named_parameters():
        if "lora_" in n and n.startswith("transformer."):
            p.requires_grad_(False)
    TestTimePromptTuner(model, learner)  # trainable image-side adapters do not matter: the image pass is the no-grad one


@pytest.mark.parametrize("V,C,d,K,seed", [(64, 403, 512, 6, 0), (5, 3, 64, 1, 3), (33, 130, 192, 3, 1), (16, 6, 64, 16, 2)])
def test_reference_gradient_is_the_closed_form(V, C, d, K, seed):
    F, T = tpt_inputs(V, C, d, seed)
    loss, dT, H, sel = tpt_ref(F, T, K, 100.0)
    assert sel.tolist() == sorted(torch.sort(H, stable=True).indices[:K].tolist())
    assert (dT - tpt_closed_form(F, T, sel, 100.0)).abs().max().item() < 1e-12
    # a given selection is used as it is
    other = torch.arange(V - K, V)
    loss2, dT2, _, sel2 = tpt_ref(F, T, K, 100.0, selected=other.flip(0))
    assert sel2.tolist() == other.tolist()
    assert (dT2 - tpt_closed_form(F, T, other, 100.0)).abs().max().item() < 1e-12
