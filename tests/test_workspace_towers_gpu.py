"""Workspace independence of the tower sequencer and the trainers: the identical call sequence runs under
``poisoned_towers`` with 0.0, NaN and 1e30 (tests/poison.py) -- every fresh allocation filled, the per-tower ``scratch``
refilled on every tower call, ``saved`` before every forward -- and every feature, logit, loss and parameter gradient
must agree bit for bit across the three fills and be finite.  After every tower call the tower's split-K counters must
be all zero (checked inside ``poisoned_towers`` at the next buffer request and here after the last call).

Each fill gets a fresh model built from the same seeds.  Two cases share frozen weights between the fills instead, to
stay quick (the 12-block ViT-B/32 text tower, the ViT-L/14-shaped fp16 model): there the ENGINE is rebuilt per fill
(``model.invalidate_engine()``: fresh scratch / saved / counters / weight planes / plan caches) and the gradients are
zeroed, so that nothing an earlier fill wrote survives.

The kernels of every path here are bitwise reproducible run to run (include/clipfs.h: no float atomics, every output
element written by one wave), so no path falls back to a tolerance."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from poison import FILLS, assert_same_runs, counters_zero, poison_, poisoned_towers, same_bits

pytestmark = pytest.mark.gpu

ATTN = {"q": "q_proj", "k": "k_proj", "v": "v_proj", "o": "proj"}
ALL6 = ("q", "k", "v", "o", "c_fc", "c_proj")
# vision 256 / text 128: widths the matrix-core adapter kernels cover, which ranks above 16 need (SMALL's 192 and TINY's
# 64 are refused there); the geometry of tests/test_lora_rank_gpu.py
RANK_CFG = dict(name="rank", embed_dim=128, image_resolution=96, vision_layers=2, vision_width=256, vision_patch_size=32,
                context_length=24, vocab_size=1024, transformer_width=128, transformer_layers=3)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _randn(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _cfg(name):
    from clipfs import synth
    return synth.ClipConfig(**RANK_CFG) if name == "RANK" else getattr(synth, name)


def _make(dev, cfg="SMALL", params=("q", "k", "v"), r=4, p=0.0, bias="none", n_vpt=0, with_ctx=False, depth=0,
          encoder="both", text_blocks=None, vision_blocks=None):
    """A fresh model with adapters on ``params`` (every A and B seeded, B non-zero), the trainable flags set."""
    import lora_train_vlp as L
    from clipfs import synth
    from jclip.model import build_model
    cfg = _cfg(cfg)
    sd = synth.synth_state_dict(cfg, seed=11, perturb=True)
    design = None
    if depth:
        design = {"vision_ctx": 4, "language_ctx": 4, "deep_prompts": True, "vision_depth": depth, "language_depth": depth}
    elif n_vpt:
        design = {"vision_ctx": n_vpt}
    model = build_model(sd, design_details=design, device=dev)
    args = types.SimpleNamespace(encoder=encoder, position="all", backbone="synthetic", params=list(params), r=r, alpha=1,
                                 dropout_rate=p)
    tb = list(range(cfg.transformer_layers)) if text_blocks is None else list(text_blocks)
    vb = list(range(cfg.vision_layers)) if vision_blocks is None else list(vision_blocks)
    saved = L.INDEX_POSITIONS_TEXT["all"]
    L.INDEX_POSITIONS_TEXT["all"] = tb
    L.INDEX_POSITIONS_VISION["synthetic"] = {"all": vb}
    try:
        layers = L.apply_lora(args, model)
    finally:
        L.INDEX_POSITIONS_TEXT["all"] = saved
        del L.INDEX_POSITIONS_VISION["synthetic"]
    rng = np.random.RandomState(5)
    with torch.no_grad():
        for layer in layers:
            for tok in params:
                m = getattr(layer, ATTN.get(tok, tok))
                fout, fin = m.w_lora_B.shape[0], m.w_lora_A.shape[1]
                m.w_lora_A.copy_(torch.from_numpy(rng.uniform(-1, 1, size=(r, fin)).astype(np.float32) / np.float32(np.sqrt(fin))))
                m.w_lora_B.copy_(torch.from_numpy((rng.standard_normal((fout, r)) * 0.05).astype(np.float32)))
    L.mark_only_lora_as_trainable(model, bias)
    if model.visual.VPT is not None:
        model.visual.VPT.requires_grad_(True)
    for n, prm in model.named_parameters():
        if n.endswith(".VPT_shallow"):
            prm.requires_grad_(True)
    model.train(p > 0)  # dropout follows the module's train mode
    ctx = torch.nn.Parameter(sd["token_embedding.weight"][[5, 6, 7, 8]].clone().to(dev)) if with_ctx else None
    return types.SimpleNamespace(L=L, cfg=cfg, model=model, layers=layers, ctx=ctx, p=p, dev=dev)


def _batch(cfg, dev, B=6, Cn=9, cap_seed=4, max_len=12, min_len=6):
    from clipfs import synth
    return (synth.synth_images(B, cfg.image_resolution, seed=3).to(dev),
            synth.synth_captions(Cn, cfg.context_length, cfg.vocab_size, seed=cap_seed, min_len=min_len, max_len=max_len).to(dev),
            synth.synth_labels(B, Cn, seed=2).to(dev))


def _three(build, run):
    """``run(build())`` under each fill; the outputs (a dict of tensors) bitwise equal and finite; returns the runs."""
    runs = []
    for fill in FILLS:
        obj = build()
        seen = []
        with poisoned_towers(fill, seen):
            out = run(obj)
            torch.cuda.synchronize()
        for rt in seen:
            assert counters_zero(rt), f"{rt.name} tower: split-K counters not zero after the last call"
        runs.append({k: torch.as_tensor(v).detach().clone() for k, v in out.items()})
    assert_same_runs(runs)
    return runs


def _rows_mode(rt, desc_args):
    from clipfs import _lib
    return _lib.load().clipfs_tower_rows_mode(C.byref(rt.descriptor(*desc_args)))


# ------------------------------------------------------------------------------------------ 1. the sequencer, directly
@pytest.mark.parametrize("stop", [False, True], ids=["to_input", "stop_at_input"])
@pytest.mark.parametrize("path", ["dense", "rows"])
@pytest.mark.parametrize("tower", ["text", "vision"])
def test_sequencer_dense_and_sparse(dev, tower, path, stop):
    """clipfs_tower_fwd + clipfs_tower_bwd, and clipfs_tower_fwd_rows + clipfs_tower_bwd_sparse, on SMALL with q / k / v
    adapters, dropout 0.25, a non-zero seed and row0.  With stop_at_input ``dx`` is documented uninitialised and is not
    compared; the gradients behind it are."""
    seed, row0, n = 0x1234567, 7, 5

    def build():
        S = _make(dev, "SMALL", p=0.25)
        S.tr = S.L.LoRATrainer(S.model)  # owns the gradient slots the descriptor points at
        return S

    def run(S):
        eng = S.model.engine
        rt = eng.txt if tower == "text" else eng.vis
        seq, d = rt.seq, rt.width
        x = _randn(n * seq, d, seed=1).to(dev)
        S.tr.flat.zero_grad()
        out = {}
        if path == "dense":
            saved = rt.forward(x, n, True, seed, row0=row0, grad_lo=0)
            assert counters_zero(rt)
            dx = _randn(n * seq, d, seed=2).to(dev)
            rt.backward(dx, n, saved, seed, stop, row0=row0, grad_lo=0)
            out["x"] = x
        else:
            assert _rows_mode(rt, (True, seed, None, row0, 0)) == 1
            rows = torch.tensor([seq - 1, 1, 8, 9, 3] if tower == "text" else [0] * n, dtype=torch.int32, device=dev)
            saved = rt.forward(x, n, True, seed, row0=row0, rows=rows, grad_lo=0)
            assert counters_zero(rt)
            dxs = _randn(n, d, seed=2).to(dev)
            dx = rt.backward_sparse(dxs, rows, n, saved, seed, stop, row0=row0, grad_lo=0)
            out["x_rows"] = x.view(n, seq, d)[torch.arange(n, device=dev), rows.long()]  # the other rows are unspecified
        assert counters_zero(rt)
        if not stop:
            out["dx"] = dx
        out["grads"] = S.tr.flat.grads
        assert bool(S.tr.flat.grads.any())
        return out

    _three(build, run)


# ------------------------------------------------------------------------------------------ 2. the packed text paths
_B32 = {}


def _b32(dev):
    """The 12-block width-512 text tower of tests/test_pack_fwd_gpu.py (ViT-B/32, rank 4 on q / k / v, dropout 0.25, train
    mode) with a trainer that owns the gradient slots; built once, its engine is rebuilt per fill."""
    if "m" not in _B32:
        import lora_train_vlp as L
        import test_pack_fwd_gpu as PF
        model, cfg = PF._model(dev)
        _B32["m"] = (model, cfg, L.LoRATrainer(model, shard_text=False), PF)
    return _B32["m"]


@pytest.mark.parametrize("table", ["eot1", "tile_edges", "mixed", "fallback"])
def test_packed_text_paths(dev, table):
    """clipfs_tower_bwd_packed over the dense records of clipfs_tower_fwd_rows, and clipfs_tower_fwd_packed +
    clipfs_tower_bwd_packed_saved, on the caption tables of tests/test_pack_fwd_gpu.py; ``fallback`` is the table where
    the library declines to pack (R > M / 2) and runs the dense rows.  dx is compared where it is formed, and its dead
    rows are exact zeros where the backward packs."""
    from clipfs import ops
    model, cfg, tr, PF = _b32(dev)
    ids = PF._table(cfg, table).to(dev)
    n, seq = ids.shape
    seed, row0 = 0x1234567, 7

    def build():
        model.invalidate_engine()
        return model.engine

    def run(eng):
        txt = eng.txt
        d = txt.width
        x0 = ops.text_embed(ids, model.token_embedding.weight.data, model.positional_embedding.data, None)
        eot = ops.eot_index(ids)
        plan, R = eng._pack_plan(ids)
        packs = txt.pack_mode(n, R, seed, seq, 0)
        assert packs == txt.pack_fwd_mode(n, R, seed, seq, 0) == (table != "fallback")
        assert _rows_mode(txt, (True, seed, seq, row0, 0)) == 1
        dxs = _randn(n, d, seed=3).to(dev)
        ar, el = torch.arange(n, device=dev), eot.long()
        dead = torch.arange(seq, device=dev)[None, :] > el[:, None]
        out = {}
        for name, pack, stop in (("dense_records", None, False), ("packed_records", (plan, R), False),
                                 ("packed_records_stop", (plan, R), True)):
            if pack is not None and not packs:
                continue  # clipfs_tower_bwd_packed_saved is refused where the forward does not pack
            x = x0.clone()
            tr.flat.zero_grad()
            saved = txt.forward(x, n, True, seed, seq, row0=row0, rows=eot, grad_lo=0, pack=pack)
            assert counters_zero(txt)
            dx = txt.backward_packed(dxs, eot, plan, R, n, saved, seed, stop, seq=seq, row0=row0, grad_lo=0,
                                     saved_packed=pack is not None)
            assert counters_zero(txt)
            out[name + ".x_eot"] = x.view(n, seq, d)[ar, el].clone()
            out[name + ".grads"] = tr.flat.grads.clone()
            assert bool(tr.flat.grads.any())
            if not stop:
                out[name + ".dx"] = dx
                if packs:
                    assert not bool(dx.view(n, seq, d)[dead].any()), "dx: dead rows must be exact zeros"
        return out

    runs = _three(build, run)
    if table != "fallback":  # the live-row forward is bitwise the dense one on the rows the head reads
        assert same_bits(runs[0]["dense_records.x_eot"], runs[0]["packed_records.x_eot"])
        assert same_bits(runs[0]["packed_records.grads"], runs[0]["packed_records_stop.grads"])


# ------------------------------------------------------------------------------------------ 3. LoRATrainer.forward_backward
# ``rows``: clipfs_tower_rows_mode of (text, vision) -- 1 = the last block runs one row per sequence (clipfs_tower_fwd_rows
# + clipfs_tower_bwd_sparse), 0 = the dense walk (an o / c_fc / c_proj adapter in the last block; TINY's 5 image tokens).
# None of these towers packs (fewer than 2048 text rows): sections 2 and 7 cover the packed walks.
TRAINER_CASES = {
    "tiny_qkv_r4": dict(cfg="TINY", rows=(1, 0)),
    "small_qkv_r4_drop": dict(cfg="SMALL", p=0.25, rows=(1, 1)),
    "tiny_qvo_r4_drop": dict(cfg="TINY", params=("q", "v", "o"), p=0.25, rows=(0, 0)),
    "small_qvo_r4": dict(cfg="SMALL", params=("q", "v", "o"), rows=(0, 0)),
    "small_all6_r4_drop": dict(cfg="SMALL", params=ALL6, p=0.25, rows=(0, 0)),
    "rank_qkv_r32_drop": dict(cfg="RANK", r=32, p=0.25, rows=(1, 1)),
    "rank_all6_r32": dict(cfg="RANK", params=ALL6, r=32, rows=(0, 0)),
    "small_ctx_vpt_drop": dict(cfg="SMALL", p=0.25, with_ctx=True, n_vpt=4, rows=(1, 1)),
    "small_deep3": dict(cfg="SMALL", with_ctx=True, depth=3, rows=(1, 1)),
    "small_bias_all_drop": dict(cfg="SMALL", p=0.25, bias="all", rows=(1, 1)),
    "small_text_up": dict(cfg="SMALL", encoder="text", text_blocks=[1, 2], rows=(1, 1)),  # a gradient floor above block 0
    "small_bf16x3_drop": dict(cfg="SMALL", p=0.25, precision="bf16x3", rows=(1, 1)),
}


def _fb(S, batch, **trainer_kw):
    """One forward_backward of a fresh trainer: loss, hit count, logits, both feature tables and the flat gradients."""
    tr = S.L.LoRATrainer(S.model, prompt_ctx=S.ctx, **trainer_kw)
    S.tr = tr
    S.model.engine.step = 3
    tr.flat.zero_grad()
    loss, correct, logits = tr.forward_backward(*batch)
    img_n, txt = tr.last_features
    assert bool(tr.flat.grads.any())
    return dict(loss=loss, correct=correct, logits=logits, img=img_n, txt=txt, grads=tr.flat.grads)


@pytest.mark.parametrize("case", sorted(TRAINER_CASES))
def test_lora_trainer_forward_backward(dev, case):
    kw = dict(TRAINER_CASES[case])
    precision, rows = kw.pop("precision", "fp32"), kw.pop("rows")

    def build():
        S = _make(dev, **kw)
        S.model.engine.precision = precision
        return S

    def run(S):
        out = _fb(S, _batch(S.cfg, dev))
        eng = S.model.engine
        assert (_rows_mode(eng.txt, (True, 1, None, 0, 0)), _rows_mode(eng.vis, (True, 1, None, 0, 0))) == rows
        n, seq = 9, S.cfg.context_length
        assert not eng.txt.pack_mode(n, n * 2, 1, seq, S.tr.last_plan["text"])
        if case == "small_text_up":
            assert S.tr.last_plan == {"text": 1, "vision": None}
        else:
            assert S.tr.last_plan == {"text": 0, "vision": 0}
        return out

    _three(build, run)


# ------------------------------------------------------------------------------------------ 4. the fp16 storage mode
_L14 = {}


def _l14(dev):
    """The ViT-L/14-shaped 2 + 2 block model of tests/test_pack_f16_gpu.py (rank 16, dropout 0.25, 32 images, prompt
    ctx): the f16 x f16 GEMMs need these widths.  Built once; engine and trainer are renewed per fill."""
    if "s" not in _L14:
        import test_pack_f16_gpu as PF16
        _L14["s"] = (PF16._Setup(dev, with_ctx=True), PF16)
    return _L14["s"]


@pytest.mark.parametrize("table", ["dense", "packed"])
def test_fp16_storage_step(dev, table):
    """A step in the fp16 storage mode under a static loss scale: ``dense`` = a caption table of which more than half
    the rows are live (the text backward runs the dense rows), ``packed`` = its backward on the live rows."""
    from clipfs import synth
    s, PF16 = _l14(dev)
    cap = PF16._captions(PF16.LENS_LONG if table == "dense" else PF16.LENS_SHORT, s.cfg.vocab_size).to(dev)
    tgt = synth.synth_labels(32, cap.shape[0], seed=2).to(dev)
    ctx = s.tr.prompt_ctx

    def build():
        s.model.invalidate_engine()
        eng = s.model.engine
        eng.precision, eng.trim_text, eng.pack_text_backward = "fp16", False, True
        return eng

    def run(eng):
        tr = s.L.LoRATrainer(s.model, prompt_ctx=ctx, shard_text=False, loss_scale=1024.0)
        eng.step = 3
        tr.flat.zero_grad()
        loss, correct, logits = tr.forward_backward(s.img, cap, tgt)
        ids, seq = eng._effective_ids(cap)
        _, R = eng._pack_plan(ids)
        assert eng.txt.pack_mode(ids.shape[0], R, 1, seq, tr.last_plan["text"]) == (table == "packed")
        assert bool(tr.flat.grads.any())
        return dict(loss=loss, correct=correct, logits=logits, grads=tr.flat.grads)

    try:
        _three(build, run)
    finally:
        s.model.invalidate_engine()
        s.model.engine.precision = "fp32"


# ------------------------------------------------------------------------------------------ 5. the fused trainers
def test_stage2_fused_step(dev):
    """One fused Stage2Trainer step (deep prompts of depth 3, frozen adapters with dropout 0.25)."""
    import test_stage2_fused_gpu as S2

    def run(s):
        loss, terms, cos = S2._step(s)
        out = dict(loss=loss, cos=cos, params=s.tr.flat.params, grads=s.tr.flat.grads)
        out.update({"term." + k: v for k, v in terms.items()})
        return out

    _three(lambda: S2._setup(dev, p=0.25, depth=3, fused=True), run)


def test_contrastive_step_pairs(dev):
    """One step_pairs (multi-positive InfoNCE over grouped pairs) on SMALL with dropout."""
    from clipfs import synth

    def run(S):
        cfg = S.cfg
        B, M = 6, 4
        img = synth.synth_images(B, cfg.image_resolution, seed=3).to(dev)
        cap = synth.synth_captions(M, cfg.context_length, cfg.vocab_size, seed=4, max_len=12).to(dev)
        ig = synth.synth_labels(B, M, seed=2).to(torch.int32).to(dev)
        cg = torch.arange(M, dtype=torch.int32, device=dev)
        tr = S.L.LoRATrainer(S.model, lr=1e-3)
        S.model.engine.step = 3
        loss, c_it, c_ti = tr.step_pairs(img, cap, ig, cg)
        return dict(loss=loss, c_it=c_it, c_ti=c_ti, params=tr.flat.params, grads=tr.flat.grads)

    _three(lambda: _make(dev, "SMALL", p=0.25), run)


def test_tpt_episode(dev):
    """One test-time prompt tuning episode over three images' view features."""
    import test_tpt_gpu as TP
    g = torch.Generator().manual_seed(2)
    feats = torch.nn.functional.normalize(torch.randn(3, 8, 128, generator=g, dtype=torch.float64), dim=-1).float().to(dev)

    def run(m):
        res = TP._tuner(m).adapt_features(feats)
        return dict(logits=res.logits, ctx=res.ctx, loss=res.loss, selected=res.selected, entropy=res.entropy,
                    ctx_grad=res.ctx_grad)

    _three(lambda: TP._build(dev), run)


def test_cache_head_trainer_step(dev):
    """One TipAdapterTrainer step (clipfs_cache_logits, cross entropy, clipfs_cache_bwd accumulating into dK, AdamW)."""
    import test_cache_head_gpu as CH
    from tip_adapter import TipAdapter, TipAdapterTrainer

    def build():
        return CH._trainer_problem(dev)

    def run(prob):
        fd, Kd, od, based, yd, _, off, labels, y = prob
        ad = TipAdapter.from_features(Kd, torch.from_numpy(labels).to(dev), 12, alpha=1.0, beta=5.5)
        tr = TipAdapterTrainer(ad, T_max=10, lr=1e-3, weight_decay=1e-2, betas=(0.9, 0.999), eps=1e-4)
        loss_sum, correct = tr.step(fd, based, yd)
        return dict(loss=loss_sum, correct=correct, keys=tr.params)

    _three(build, run)


def test_modified_resnet_trainer_step(dev):
    """One LoRATrainer step with the RN_TINY ModifiedResNet image tower, whose activation buffers clipfs/resnet.py
    allocates itself (text adapters with dropout, prompt ctx)."""
    import test_modified_resnet_gpu as RN

    def run(S):
        img, cap, tgt = (t.to(dev) for t in RN._batch(S.geo))
        S.model.train()
        tr = S.L.LoRATrainer(S.model, prompt_ctx=S.ctx)
        S.model.engine.step = 3
        loss, correct, logits = tr.step(img, cap, tgt)
        return dict(loss=loss, correct=correct, logits=logits, params=tr.flat.params, grads=tr.flat.grads)

    _three(lambda: RN._make_trainable(dev, 0.25, True), run)


# ------------------------------------------------------------------------------------------ 6. the autograd route
def test_autograd_route_two_text_forwards(dev):
    """encode_text twice with gradients enabled (two caption chunks, each with its own saved tensor) and encode_image
    before ONE backward: the second forward must not disturb what the first one saved."""
    from clipfs import engine as E

    def run(S):
        img, cap, tgt = _batch(S.cfg, dev)
        Cn = cap.shape[0]
        S.model.engine.step = 3
        emb = torch.cat([S.model.encode_text(cap[:5].contiguous()), S.model.encode_text(cap[5:].contiguous())])
        txt = E.class_mean(emb, Cn, 1)
        fi = E.l2_normalize(S.model.encode_image(img))
        logits = E.cosine_logits(fi, txt, 100.0)
        loss = E.cross_entropy_loss(logits, tgt)
        loss.backward()
        out = dict(loss=loss.detach(), logits=logits.detach())
        params = S.L.get_lora_parameters(S.model)
        assert params and all(p.grad is not None for p in params)
        out.update({f"grad{i}": p.grad for i, p in enumerate(params)})
        return out

    _three(lambda: _make(dev, "SMALL", p=0.25), run)


# ------------------------------------------------------------------------------------------ 7. stale shapes on one trainer
def _poison_tower_buffers(eng, fill):
    """What a skipped overflow step leaves behind: the cached scratch and saved tensors of both towers hold ``fill``."""
    for rt in (eng.txt, eng.vis):
        for (kind, _), buf in rt._bufs.items():
            if kind in ("scratch", "saved"):
                poison_(buf, fill)


@pytest.mark.parametrize("poison_between", [False, True], ids=["plain", "nan_step_between"])
def test_stale_shape_sequence(dev, poison_between):
    """One trainer, no optimiser step in between: forward_backward at batch 6 over caption table A, at batch 3 over a
    table B with other caption lengths (another packed plan, other buffer sizes), at batch 6 over A again.  The third
    result is bitwise the first, the second bitwise that of a fresh trainer.  96 captions of at most 12 of 24 tokens:
    2304 text rows, of which fewer than half are live, so that the text backward packs.  ``nan_step_between``: before
    the last call every cached scratch / saved tensor is filled with NaN, as after a skipped fp16 overflow step."""
    def tables(S):
        a = _batch(S.cfg, dev, B=6, Cn=96, cap_seed=4, max_len=9, min_len=2)
        b = _batch(S.cfg, dev, B=3, Cn=96, cap_seed=8, max_len=5, min_len=1)
        return a, b

    def one(tr, S, batch):
        S.model.engine.step = 3
        tr.flat.zero_grad()
        loss, correct, logits = tr.forward_backward(*batch)
        torch.cuda.synchronize()
        eng = S.model.engine
        _, R = eng._pack_plan(batch[1])
        n, seq = batch[1].shape
        assert eng.txt.pack_mode(n, R, 1, seq, tr.last_plan["text"]), "the text backward is meant to pack here"
        return dict(loss=loss.clone(), logits=logits.clone(), grads=tr.flat.grads.clone())

    S = _make(dev, "SMALL", p=0.25, with_ctx=True)
    a, b = tables(S)
    assert a[1].shape == b[1].shape and not torch.equal(a[1].argmax(-1), b[1].argmax(-1))
    tr = S.L.LoRATrainer(S.model, prompt_ctx=S.ctx, shard_text=False)
    first = one(tr, S, a)
    second = one(tr, S, b)
    if poison_between:
        _poison_tower_buffers(S.model.engine, float("nan"))
    third = one(tr, S, a)
    F = _make(dev, "SMALL", p=0.25, with_ctx=True)
    fresh = one(F.L.LoRATrainer(F.model, prompt_ctx=F.ctx, shard_text=False), F, tables(F)[1])
    assert_same_runs([first, third], ids=("first call", "third call"))
    assert_same_runs([fresh, second], ids=("fresh trainer", "second call"))
    for rt in (S.model.engine.txt, S.model.engine.vis):
        assert counters_zero(rt)
