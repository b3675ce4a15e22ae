"""Merged-weight evaluation and export on the GPU: clipfs_lora_merge against fp64, its 16-bit planes against the stand-alone
converters, the merged towers against the fp64 oracle's additive form, the fast paths an MLP adapter costs and merging
gives back, the fp16 storage mode, state handling, refusals, the plain-checkpoint export and evaluate_lora(merged=True).

Bounds.  Kernel: |out - (W + s B A)| <= (r + 3) 2^-24 (|W| + |s| sum_j |B_nj A_jk|) elementwise, right-hand side in fp64:
the rank sum is sequential with one fused multiply-add per step (r roundings on the running sum), then one more for
fma(s, acc, W); nothing is measured.  Towers: 100 x cosine logits within 1e-3 of the oracle, the standing bound of the
adapter path (tests/test_mlp_lora_gpu.py).  fp16 storage mode: 2e-2 on the logits, the mode's stated budget
(tests/test_golden_gpu.py).  evaluate_views logits, merged against the adapter path: 2e-3, two 1e-3 bounds around the
same fp64 value.  Everything else is bitwise."""
import dataclasses
import hashlib
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ATTN = {"q": "q_proj", "k": "k_proj", "v": "v_proj", "o": "proj"}
ALL6 = ("q", "k", "v", "o", "c_fc", "c_proj")
# (n, k, nseg, seg_mask): ragged rows (72 = 2 tiles + 8), ragged columns (40, 64, 192 against 256-column tiles), several
# column tiles (512, 1024), segments with and without an adapter, and one job of many tiles
SHAPES = [(192, 64, 3, 0b111), (576, 192, 3, 0b101), (512, 128, 1, 1), (128, 512, 1, 1), (72, 40, 1, 1), (3072, 1024, 3, 0b010)]
RANKS = [4, 16, 1, 64, 3, 17]  # the rank each shape is listed with; every call below carries all six shapes at one rank
SENTINEL, GUARD = 1234.5, 64   # 64 floats (256 bytes) on both sides of every output


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _leave_the_global_generators_alone():
    """Some tests that run after this file draw from torch's global generators (nn.Linear's own initialisation in the
    stage-2 heads) and their margins depend on the values drawn: every test here hands the generators back as it found
    them, so those tests see the stream they saw before this file existed."""
    import random
    cpu, py, npy = torch.get_rng_state(), random.getstate(), np.random.get_state()
    gpu = torch.cuda.get_rng_state_all() if torch.cuda.is_available() else None
    yield
    torch.set_rng_state(cpu)
    random.setstate(py)
    np.random.set_state(npy)
    if gpu is not None:
        torch.cuda.set_rng_state_all(gpu)


def _err(got, want):
    return (got.detach().double().cpu() - want.detach().double().cpu()).abs().max().item()


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------------------------------------------------

def _inputs(r, zero_b=False):
    rng = np.random.RandomState(100 + r)
    out = []
    for n, k, nseg, mask in SHAPES:
        w = (rng.standard_normal((n, k)) * 0.02).astype(np.float32)
        a = (rng.uniform(-1, 1, size=(nseg * r, k)) / np.sqrt(k)).astype(np.float32)
        b = (rng.standard_normal((n, r)) * 0.02).astype(np.float32)
        out.append((w, a, b * 0 if zero_b else b))
    return out


def _guarded(dev, n_bytes, dtype):
    """A tensor of ``n_bytes`` with GUARD sentinel floats before and after it: (whole buffer as bytes, the inner view)."""
    g = GUARD * 4
    buf = torch.empty(g + n_bytes + g, device=dev, dtype=torch.uint8)
    buf.view(torch.float32)[:] = SENTINEL
    return buf, buf[g:g + n_bytes].view(dtype)


def _guards_intact(buf, n_bytes):
    g = GUARD * 4
    f = buf.view(torch.float32)
    return bool((f[:GUARD] == SENTINEL).all() and (f[(g + n_bytes) // 4:] == SENTINEL).all())


def _run(dev, host, r, scale, fmt):
    """One clipfs_lora_merge call over all six shapes: [(out, planes | None)], after checking the guards and the inputs."""
    from clipfs import ops
    jobs, keep = [], []
    for (w, a, b), (n, k, nseg, mask) in zip(host, SHAPES):
        W, A, B = (torch.from_numpy(v).to(dev) for v in (w, a, b))
        obuf, out = _guarded(dev, n * k * 4, torch.float32)
        pbuf = planes = None
        if fmt:
            pbuf, planes = _guarded(dev, n * k * (4 if fmt == 1 else 2), torch.int16)
        jobs.append((W, A, B, nseg, mask, out.view(n, k), planes))
        keep.append((W, A, B, obuf, pbuf))
    assert len(jobs) >= 3
    ops.lora_merge(jobs, r, scale, fmt)
    torch.cuda.synchronize()
    res = []
    for (w, a, b), (n, k, nseg, mask), job, (W, A, B, obuf, pbuf) in zip(host, SHAPES, jobs, keep):
        assert _guards_intact(obuf, n * k * 4), f"out guards of {(n, k)} at r {r}"
        if fmt:
            assert _guards_intact(pbuf, n * k * (4 if fmt == 1 else 2)), f"plane guards of {(n, k)} at r {r}"
        for t, h, what in ((W, w, "W"), (A, a, "A"), (B, b, "B")):
            assert torch.equal(t.cpu(), torch.from_numpy(h)), f"{what} of {(n, k)} was written"
        res.append((job[5], job[6]))
    return res


@pytest.mark.parametrize("r", RANKS)
def test_kernel_against_fp64(dev, r):
    """All six shapes as ONE table per call, at each of the ranks: the job lookup, every row / column / segment tail."""
    from clipfs import ops
    scale = float(np.float32(1.0 / np.sqrt(r)))
    host = _inputs(r)
    plain = _run(dev, host, r, scale, 0)
    for (w, a, b), (n, k, nseg, mask), (out, _) in zip(host, SHAPES, plain):
        got = out.cpu().numpy()
        d = n // nseg
        w64, want, mag = w.astype(np.float64), np.empty((n, k)), np.empty((n, k))
        for g in range(nseg):
            rows, ag = slice(g * d, (g + 1) * d), a[g * r:(g + 1) * r].astype(np.float64)
            bg = b[rows].astype(np.float64)
            if (mask >> g) & 1:
                want[rows] = w64[rows] + scale * (bg @ ag)
                mag[rows] = np.abs(w64[rows]) + abs(scale) * (np.abs(bg) @ np.abs(ag))
            else:  # no adapter on this segment: the bits of W
                want[rows], mag[rows] = w64[rows], 0.0
                assert np.array_equal(got[rows].view(np.int32), w[rows].view(np.int32)), f"{(n, k)} segment {g} is not W"
        excess = np.abs(got.astype(np.float64) - want) - (r + 3) * 2.0 ** -24 * mag
        moved = np.abs(want - w64).max()
        print(f"r {r} {(n, k)} mask {mask:#b}: max err {np.abs(got - want).max():.3e}, worst err / bound "
              f"{(np.abs(got - want) / np.maximum((r + 3) * 2.0 ** -24 * mag, 1e-300)).max():.3f}, adapter moves W by {moved:.3e}")
        assert excess.max() <= 0, f"r {r} {(n, k)}: {excess.max():.3e} over the bound"
        assert moved > 1e-4, "the adapter must move the weight (the test is vacuous otherwise)"
    # planes: the same out, and bit for bit what the stand-alone converters make of it
    for fmt in (1, 2):
        res = _run(dev, host, r, scale, fmt)
        for (n, k, _, _), (out, planes), (ref, _) in zip(SHAPES, res, plain):
            assert torch.equal(out, ref), f"out depends on the plane format ({(n, k)}, format {fmt})"
            want = ops.split_bf16(out.contiguous()) if fmt == 1 else ops.to_f16(out.contiguous()).view(torch.int16)
            assert torch.equal(planes.view(want.shape), want), f"planes of {(n, k)} in format {fmt}"
    # two runs: bitwise
    for (out, _), (ref, _) in zip(_run(dev, host, r, scale, 0), plain):
        assert torch.equal(out, ref)


@pytest.mark.parametrize("r", [3, 16])
def test_zero_b_is_the_identity(dev, r):
    host = _inputs(r, zero_b=True)
    for (w, _, _), (out, planes) in zip(host, _run(dev, host, r, 0.5, 2)):
        assert np.abs(w).max() > 0
        assert np.array_equal(out.cpu().numpy().view(np.int32), w.view(np.int32))
        assert torch.equal(planes.view(torch.float16).view(out.shape).cpu(), torch.from_numpy(w).half())


# ---------------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------------

def _adapt(model, cfg, params, r, p=0.0, encoder="both", seed=5):
    """apply_lora on every block with every A and B random (B non-zero); returns (L, layers)."""
    import lora_train_vlp as L
    args = types.SimpleNamespace(encoder=encoder, position="all", backbone="synthetic", params=list(params), r=r, alpha=1,
                                 dropout_rate=p)
    saved = L.INDEX_POSITIONS_TEXT["all"]
    L.INDEX_POSITIONS_TEXT["all"] = list(range(cfg.transformer_layers))
    L.INDEX_POSITIONS_VISION["synthetic"] = {"all": list(range(cfg.vision_layers))}
    try:
        layers = L.apply_lora(args, model)
    finally:
        L.INDEX_POSITIONS_TEXT["all"] = saved
        del L.INDEX_POSITIONS_VISION["synthetic"]
    rng = np.random.RandomState(seed)
    with torch.no_grad():
        for layer in layers:
            for tok in params:
                m = getattr(layer, ATTN.get(tok, tok))
                fout, fin = m.w_lora_B.shape[0], m.w_lora_A.shape[1]
                m.w_lora_A.copy_(torch.from_numpy(rng.uniform(-1, 1, size=(r, fin)).astype(np.float32) / np.float32(np.sqrt(fin))))
                m.w_lora_B.copy_(torch.from_numpy((rng.standard_normal((fout, r)) * 0.05).astype(np.float32)))
    L.mark_only_lora_as_trainable(model)
    return L, layers


def _small(dev, params=ALL6, r=4, p=0.0, cfg_name="TINY", encoder="both"):
    from clipfs import synth
    from jclip.model import build_model
    cfg = getattr(synth, cfg_name)
    sd = synth.synth_state_dict(cfg, seed=11, perturb=True)
    model = build_model(sd, device=dev)
    L, layers = _adapt(model, cfg, params, r, p, encoder)
    return types.SimpleNamespace(L=L, cfg=cfg, sd=sd, model=model, layers=layers)


def _batch(cfg, dev, B=6, Cn=9):
    from clipfs import synth
    return (synth.synth_images(B, cfg.image_resolution, seed=3).to(dev),
            synth.synth_captions(Cn, cfg.context_length, cfg.vocab_size, seed=4, max_len=12).to(dev))


@torch.no_grad()
def _logits(model, img, cap):
    """100 x cosine logits from the drop-in encoders, as LoRATrainer forms them with one template per class."""
    from clipfs import engine as E
    txt = E.class_mean(model.encode_text(cap), cap.shape[0], 1)
    return E.cosine_logits(E.l2_normalize(model.encode_image(img)), txt, 100.0)


def _state_hash(model):
    """sha256 over every parameter (master weights, biases, adapter views) and the stacked weight / adapter tensors."""
    h = hashlib.sha256()
    for n, p in sorted(model.named_parameters()):
        h.update(n.encode() + p.detach().cpu().numpy().tobytes())
    for blk in list(model.transformer.resblocks) + list(getattr(model.visual, "transformer", model.transformer).resblocks):
        a = blk.attn
        for name in ("qkv_weight", "qkv_bias", "lora_A_qkv", "lora_B_qkv", "lora_A_o", "lora_B_o"):
            if hasattr(a, name):
                h.update(getattr(a, name).detach().cpu().numpy().tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------------------------------------------------------------
# 2. merged towers against the fp64 oracle
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r", [4, 16])
@pytest.mark.parametrize("params", [("q", "k", "v"), ("q", "v", "o"), ALL6], ids=lambda v: "-".join(v))
@pytest.mark.parametrize("cfg_name", ["TINY", "SMALL"])
def test_merged_towers_against_the_oracle(dev, monkeypatch, cfg_name, params, r):
    """Eval mode, B non-zero: the oracle's additive form at p = 0 (it forms B @ A like merge_BA) is the reference for the
    merged towers, in fp32 and in bf16x3 (the same bound); the adapter path's error is printed beside the merged one."""
    import test_mlp_lora_gpu as T
    from oracle import clip_oracle as O
    monkeypatch.setattr(O, "resblock_forward", T._resblock)
    S = T._make(dev, cfg_name, params, p=0.0, r=r)
    img, cap, tgt = T._batch(S.cfg)
    with torch.no_grad():
        _, want = T._oracle_loss(S, T._oracle_state(S), img, cap, tgt, 0)
    img, cap = img.to(dev), cap.to(dev)
    S.model.eval()
    adapter = _logits(S.model, img, cap)
    n_proj = len(params) * (S.cfg.transformer_layers + S.cfg.vision_layers)
    assert S.L.merge_lora(S.model) == n_proj and S.model.engine.merged
    merged = _logits(S.model, img, cap)
    S.model.engine.precision = "bf16x3"  # the missing planes are built from the merged fp32 copy
    merged_bf16 = _logits(S.model, img, cap)
    S.L.merge_lora(S.model)              # ... or by the merge kernel itself: the same bits
    assert torch.equal(_logits(S.model, img, cap), merged_bf16)
    S.model.engine.precision = "fp32"
    S.L.unmerge_lora(S.model)
    # without the adapters the logits are far outside the bound: the merge is what the test sees
    with torch.no_grad():
        for layer in S.layers:
            for tok in params:
                getattr(layer, T._oname(tok)).w_lora_B.zero_()
    bare = _logits(S.model, img, cap)
    e_a, e_m, e_b = _err(adapter, want), _err(merged, want), _err(merged_bf16, want)
    print(f"{cfg_name} {'-'.join(params)} r {r}: logits err merged {e_m:.3e}, adapter path {e_a:.3e}, merged bf16x3 {e_b:.3e}; "
          f"adapters move the logits by {_err(bare, want):.3e}")
    assert _err(bare, want) > 1e-2, "the adapters must change the logits (the test is vacuous otherwise)"
    assert e_m <= 1e-3 and e_b <= 1e-3, (e_m, e_b)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the fast paths come back
# ---------------------------------------------------------------------------------------------------------------------

def test_text_fast_paths_return(dev):
    """A text tower with c_fc / c_proj adapters at the width, sequence length and caption lengths of
    tests/test_pack_fwd_gpu.py (60 captions = 4620 dense rows; the packed forward needs 2048): unmerged, the live-row
    forward and the one-row last block are off; merged, both answer as for the same model without adapters, and the
    packed merged features are bitwise the dense merged ones."""
    import ctypes

    import test_pack_fwd_gpu as P
    from clipfs import _lib, synth
    from jclip.model import build_model
    cfg = dataclasses.replace(synth.VIT_B32, vision_layers=1, transformer_layers=3)
    sd = synth.synth_state_dict(cfg, seed=1234)
    plain = build_model(sd, device=dev)
    model = build_model(sd, device=dev)
    L, _ = _adapt(model, cfg, ("c_fc", "c_proj"), 4, encoder="text")
    model.eval()
    rs = np.random.RandomState(11)
    ids = P._captions([77, 2, 33] + [int(v) for v in rs.randint(2, 30, size=57)]).to(dev)
    n = ids.shape[0]

    def modes(m):
        eng = m.engine
        _, R = eng._pack_plan(ids)
        desc = eng.txt.descriptor(False, 0, 77)
        return (eng.txt.pack_fwd_mode(n, R, 0, 77, 0, train=False), int(_lib.load().clipfs_tower_rows_mode(ctypes.byref(desc))))

    want = modes(plain)
    assert want[0] and want[1] != 0
    assert modes(model) == (False, 0)
    assert L.merge_lora(model) == 2 * cfg.transformer_layers
    assert modes(model) == want
    feats = {}
    for fwd in (True, False):
        model.engine.pack_text_forward = fwd
        with torch.no_grad():
            feats[fwd] = model.encode_text(ids).clone()
    model.engine.pack_text_forward = True
    assert torch.equal(feats[True], feats[False])
    L.unmerge_lora(model)
    with torch.no_grad():
        adapter = model.encode_text(ids)
    assert modes(model) == (False, 0)
    # the merged features are the adapter path's up to rounding, and not the unadapted model's
    with torch.no_grad():
        bare = plain.encode_text(ids)
    rel = lambda a, b: ((a - b).norm() / b.norm()).item()
    print(f"merged vs adapter path {rel(feats[True], adapter):.3e}, adapter vs no adapter {rel(bare, adapter):.3e}")
    assert rel(feats[True], adapter) < 1e-4 < 1e-2 < rel(bare, adapter)


# ---------------------------------------------------------------------------------------------------------------------
# 4. fp16 storage mode
# ---------------------------------------------------------------------------------------------------------------------

def test_fp16_mode_runs_merged_mlp_adapters(dev):
    """The smallest geometry the fp16-mode tests run (tests/test_stage2_fused_gpu.py: ViT-L/14 widths, two blocks per
    tower, 4 images, 6 captions) with all six adapters: refused unmerged exactly as test_fp16_mode_refuses_mlp_adapters
    pins, inside the mode's 2e-2 budget of the fp32 merged logits once merged -- merged before or after the switch."""
    from clipfs import synth
    from clipfs._lib import ClipfsError
    from jclip.model import build_model
    cfg = dataclasses.replace(synth.VIT_L14, vision_layers=2, transformer_layers=2, vocab_size=2048)
    model = build_model(synth.synth_state_dict(cfg, seed=17), device=dev)
    L, _ = _adapt(model, cfg, ALL6, 16)
    model.eval()
    img = synth.synth_images(4, cfg.image_resolution, seed=3).to(dev)
    cap = synth.synth_captions(6, cfg.context_length, cfg.vocab_size, seed=4, max_len=20).to(dev)
    L.merge_lora(model)
    want = _logits(model, img, cap)
    model.engine.precision = "fp16"          # merged in fp32: the f16 planes come from the merged copy on first use
    late = _logits(model, img, cap)
    L.merge_lora(model)                      # merged in fp16: the kernel writes them
    got = _logits(model, img, cap)
    assert torch.equal(got, late)
    print(f"fp16 storage mode, merged: logits err {_err(got, want):.3e} against fp32 merged (budget 2e-2)")
    assert 0 < _err(got, want) <= 2e-2
    L.unmerge_lora(model)
    with pytest.raises(ClipfsError, match=r"block 0 has a c_fc adapter"):
        with torch.no_grad():
            model.encode_image(img)
    with pytest.raises(ClipfsError, match=r"block 0 has a c_fc adapter"):
        with torch.no_grad():
            model.encode_text(cap)
    model.engine.precision = "fp32"


# ---------------------------------------------------------------------------------------------------------------------
# 5. state
# ---------------------------------------------------------------------------------------------------------------------

def test_state_is_never_written(dev):
    S = _small(dev)
    img, cap = _batch(S.cfg, dev)
    S.model.eval()
    layers = [m for m in S.model.modules() if isinstance(m, S.L.LoRALayer)]
    assert layers and not any(m.merged for m in layers) and not S.model.engine.merged
    h0 = _state_hash(S.model)
    with torch.no_grad():
        fi0, ft0 = S.model.encode_image(img).clone(), S.model.encode_text(cap).clone()
    n = S.L.merge_lora(S.model)
    assert n == 6 * (S.cfg.transformer_layers + S.cfg.vision_layers)
    assert all(m.merged for m in layers) and S.model.engine.merged
    with torch.no_grad():
        fi1 = S.model.encode_image(img).clone()
    assert not torch.equal(fi1, fi0)  # another path ran
    assert S.L.merge_lora(S.model) == n  # refresh
    h1 = _state_hash(S.model)
    S.L.unmerge_lora(S.model)
    assert not any(m.merged for m in layers) and not S.model.engine.merged
    h2 = _state_hash(S.model)
    assert h0 == h1 == h2
    with torch.no_grad():
        assert torch.equal(S.model.encode_image(img), fi0) and torch.equal(S.model.encode_text(cap), ft0)
    # the context manager restores the state, also on an exception and inside an outer merge
    with pytest.raises(RuntimeError, match="boom"):
        with S.L.merged_lora(S.model):
            assert S.model.engine.merged and all(m.merged for m in layers)
            raise RuntimeError("boom")
    assert not S.model.engine.merged and not any(m.merged for m in layers)
    S.L.merge_lora(S.model)
    with S.L.merged_lora(S.model):
        pass
    assert S.model.engine.merged and all(m.merged for m in layers)
    S.L.unmerge_lora(S.model)
    # a refresh picks the current adapter values up
    with S.L.merged_lora(S.model):
        with torch.no_grad():
            a = S.model.encode_text(cap).clone()
            S.layers[0].c_fc.w_lora_B.mul_(2.0)
            assert torch.equal(S.model.encode_text(cap), a)  # the copy, until refreshed
            S.L.merge_lora(S.model)
            assert not torch.equal(S.model.encode_text(cap), a)


def test_model_without_adapters(dev):
    import lora_train_vlp as L
    from clipfs import synth
    from jclip.model import build_model
    model = build_model(synth.synth_state_dict(synth.TINY, seed=11), device=dev)
    assert L.merge_lora(model) == 0 and not model.engine.merged
    L.unmerge_lora(model)


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals while merged
# ---------------------------------------------------------------------------------------------------------------------

def test_refusals_while_merged(dev, tmp_path):
    S = _small(dev, p=0.25)
    img, cap = _batch(S.cfg, dev)
    tgt = torch.zeros(img.shape[0], dtype=torch.long, device=dev)
    tr = S.L.LoRATrainer(S.model)
    S.L.merge_lora(S.model)
    S.model.train()
    with torch.no_grad():  # a train-mode forward of the additive form would drop
        with pytest.raises(ValueError, match="unmerge_lora"):
            S.model.encode_image(img)
        with pytest.raises(ValueError, match="unmerge_lora"):
            S.model.encode_text(cap)
    with pytest.raises(ValueError, match="unmerge_lora"):  # the autograd route with a trainable adapter
        S.model.encode_text(cap)
    S.model.eval()
    with pytest.raises(ValueError, match="unmerge_lora"):
        S.model.encode_image(img)
    with pytest.raises(ValueError, match="unmerge_lora"):
        tr.forward_backward(img, cap, tgt)
    with pytest.raises(ValueError, match="unmerge_lora"):
        tr.step(img, cap, tgt)
    with pytest.raises(ValueError, match="unmerge_lora"):  # building a trainer would re-home the adapters
        S.L.LoRATrainer(S.model)
    assert S.model.engine.merged
    # load_lora writes adapter values: it leaves the model unmerged
    args = types.SimpleNamespace(encoder="both", position="all", params=list(ALL6), r=4, alpha=1)
    path = str(tmp_path / "lora.pkl")
    S.L.save_lora(args, 0, S.layers, path)
    assert S.model.engine.merged  # saving writes what it writes today
    S.L.load_lora(args, S.layers, path)
    assert not S.model.engine.merged and not any(m.merged for m in S.model.modules() if isinstance(m, S.L.LoRALayer))
    tr.forward_backward(img, cap, tgt)  # and trains again


def test_train_mode_without_dropout_is_allowed(dev):
    S = _small(dev, p=0.0)
    img, cap = _batch(S.cfg, dev)
    S.L.merge_lora(S.model)
    S.model.eval()
    with torch.no_grad():
        want = S.model.encode_image(img).clone(), S.model.encode_text(cap).clone()
        S.model.train()
        assert torch.equal(S.model.encode_image(img), want[0]) and torch.equal(S.model.encode_text(cap), want[1])


def test_fused_stage2_is_refused_while_merged(dev):
    import test_stage2_fused_gpu as T2
    for fused in (True, False):
        s = T2._setup(dev, p=0.25, fused=fused)
        import lora_train_vlp as L
        assert L.merge_lora(s.model) > 0
        with pytest.raises(ValueError, match="unmerge_lora"):
            T2._step(s)
        L.unmerge_lora(s.model)
        T2._step(s)


# ---------------------------------------------------------------------------------------------------------------------
# 7. export
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("params", [("q", "v"), ALL6], ids=lambda v: "-".join(v))
def test_merged_state_dict_round_trip(dev, params):
    from jclip.model import build_model
    S = _small(dev, params=params, cfg_name="SMALL")
    img, cap = _batch(S.cfg, dev)
    S.model.eval()
    sd = S.L.merged_state_dict(S.model)
    assert not S.model.engine.merged  # left as found
    assert not [k for k in sd if "lora" in k]
    assert all(v.device.type == "cpu" and v.dtype == torch.float32 for v in sd.values())
    assert sorted(sd) == sorted(S.sd), "exactly the keys of the plain checkpoint the model was built from"
    plain = build_model(sd, device=dev)
    with S.L.merged_lora(S.model), torch.no_grad():
        fi, ft = S.model.encode_image(img).clone(), S.model.encode_text(cap).clone()
    with torch.no_grad():
        assert torch.equal(plain.encode_image(img), fi) and torch.equal(plain.encode_text(cap), ft)
        assert not torch.equal(build_model(S.sd, device=dev).encode_text(cap), ft)  # the adapters are in it


def test_merged_state_dict_refuses_prompts(dev):
    import lora_train_vlp as L
    from clipfs import synth
    from jclip.model import build_model
    sd = synth.synth_state_dict(synth.TINY, seed=11)
    model = build_model(sd, design_details={"vision_ctx": 4}, device=dev)
    with pytest.raises(ValueError, match="VPT"):
        L.merged_state_dict(model)
    deep = build_model(sd, design_details={"vision_ctx": 0, "deep_prompts": True, "language_depth": 2, "language_ctx": 2},
                       device=dev)
    with pytest.raises(ValueError, match="deep prompts"):
        L.merged_state_dict(deep)
    with pytest.raises(ValueError, match="prompt ctx"):
        L.merged_state_dict(build_model(sd, device=dev), prompt_ctx=torch.zeros(4, 64))


def test_resnet_model_merges_its_text_tower(dev):
    """An RN50-family model has adapters on the text tower only: merged, its text features give the adapter path's logits
    within the 1e-3 bound, and the export round-trips."""
    import modified_resnet_ref as R
    from jclip.model import build_model
    geo = R.geometries()["RN_TINY"]
    sd = R.synth_sd(geo)
    model = build_model(sd, device=dev)
    L, layers = _adapt(model, geo.text, ("q", "v", "c_fc"), 4, encoder="text")
    model.eval()
    from clipfs import synth
    img = synth.synth_images(4, geo.resolution, seed=3).to(dev)
    cap = synth.synth_captions(9, geo.text.context_length, geo.text.vocab_size, seed=4, max_len=12).to(dev)
    adapter = _logits(model, img, cap)
    assert L.merge_lora(model) == 3 * geo.text.transformer_layers
    merged = _logits(model, img, cap)
    plain = build_model(L.merged_state_dict(model), device=dev)
    assert torch.equal(_logits(plain, img, cap), merged)
    L.unmerge_lora(model)
    with torch.no_grad():
        for layer in layers:
            for name in ("q_proj", "v_proj", "c_fc"):
                getattr(layer, name).w_lora_B.zero_()
    bare = _logits(model, img, cap)
    print(f"RN text tower: merged vs adapter path {_err(merged, adapter):.3e}, adapters move the logits by {_err(bare, adapter):.3e}")
    assert _err(merged, adapter) <= 1e-3 < 1e-2 < _err(bare, adapter)


# ---------------------------------------------------------------------------------------------------------------------
# 8. evaluate_lora(merged=True)
# ---------------------------------------------------------------------------------------------------------------------

def test_evaluate_lora_merged(dev):
    from clipfs import ops, synth
    S = _small(dev, cfg_name="SMALL")
    cfg = S.cfg
    V = 5  # the centre view and four crops: the fewest views the MTA kernel takes
    views = synth.synth_images(6 * V, cfg.image_resolution, seed=8).reshape(6, V, 3, cfg.image_resolution, cfg.image_resolution)
    target = synth.synth_labels(6, 9, seed=2)
    loader = [(views[i:i + 3, 0], views[i:i + 3, 1:], target[i:i + 3], None) for i in (0, 3)]
    cap = synth.synth_captions(9, cfg.context_length, cfg.vocab_size, seed=4, max_len=12).to(dev)
    S.model.eval()
    with torch.no_grad():
        text = ops.l2norm_fwd(S.model.encode_text(cap)).t().contiguous()  # [d, C] unit columns
    args = types.SimpleNamespace()

    @torch.no_grad()
    def view_logits():  # the three logit sets evaluate_views ranks
        fv = ops.l2norm_fwd(S.model.encode_image(views.reshape(6 * V, *views.shape[2:]).to(dev)).contiguous()).reshape(6, V, -1)
        tcd = text.t().contiguous()
        return (ops.mta(fv, tcd, want_mode=False)[1], 100.0 * ops.gemm_nt(fv[:, 0].contiguous(), tcd),
                100.0 * ops.gemm_nt(fv.mean(dim=1).contiguous(), tcd))

    res = S.L.evaluate_lora(args, S.model, loader, textual_features=text)
    res_m = S.L.evaluate_lora(args, S.model, loader, textual_features=text, merged=True)
    assert isinstance(res_m, tuple) and len(res_m) == 3 and all(0.0 <= v <= 100.0 for v in res_m)
    assert not S.model.engine.merged  # left as found ...
    la = view_logits()
    S.L.merge_lora(S.model)
    res_mm = S.L.evaluate_lora(args, S.model, loader, textual_features=text, merged=True)
    assert S.model.engine.merged      # ... merged when it was merged
    lm = view_logits()
    S.L.unmerge_lora(S.model)
    assert res_mm == res_m
    errs = [_err(a, b) for a, b in zip(lm, la)]
    print(f"evaluate_views logits (mta, centre, ensemble), merged vs adapter path: {errs}; accuracies {res} / {res_m}")
    assert max(errs) <= 2e-3
