"""Packed (live-row) text backward (clipfs_tower_bwd_packed, Engine.pack_text_backward) against the all-rows backward.

The forward is the same in both runs, so loss and logits are bitwise equal.  Parameter gradients differ only in the
summation order of their row reductions (the packed run leaves out exact-zero rows): the budget is 1e-5 of each
compared tensor's largest magnitude (at least 1e-3 of the largest gradient, for gradients that cancel to rounding).  Two packed runs are bitwise equal."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAMES = {"q": "q_proj", "k": "k_proj", "v": "v_proj", "o": "proj"}
REL = 1e-5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _captions(lens, vocab=49408, seq=77, seed=9):
    """ids [n, seq] with caption c's EOT at position lens[c] - 1 (lens[c] >= 2: SOT ... EOT)."""
    rng = np.random.RandomState(seed)
    out = np.zeros((len(lens), seq), dtype=np.int64)
    for c, n in enumerate(lens):
        out[c, 0] = vocab - 2
        out[c, 1:n - 1] = rng.randint(1, vocab - 2, size=n - 2)
        out[c, n - 1] = vocab - 1
    return torch.from_numpy(out)


def _model(dev, position="all", bias="none", p=0.25, freeze_text=False):
    import lora_train_vlp as L
    from clipfs import synth
    from jclip.model import build_model
    cfg = synth.VIT_B32
    model = build_model(synth.synth_state_dict(cfg, seed=1234), device=dev)
    args = types.SimpleNamespace(encoder="both" if position == "all" else "text", position=position, backbone="ViT-B/32",
                                 params=["q", "k", "v"], r=4, alpha=1, dropout_rate=p)
    layers = L.apply_lora(args, model)
    lw = synth.synth_lora(cfg, 4, seed=5)
    with torch.no_grad():
        for i, layer in enumerate(layers):
            ab = lw.get(f"layer_{i}")
            if ab is None:
                continue
            for pr in "qkv":
                m = getattr(layer, NAMES[pr])
                m.w_lora_A.copy_(torch.from_numpy(ab[NAMES[pr]]["w_lora_A"]))
                m.w_lora_B.copy_(torch.from_numpy(ab[NAMES[pr]]["w_lora_B"]))
    L.mark_only_lora_as_trainable(model, bias)
    if freeze_text:
        for layer in layers[:12]:
            for prm, _ in layer.trainable_pairs():
                prm.requires_grad_(False)
    model.train()
    return model, cfg


def _run(dev, model, cfg, cap, with_ctx=True, n_img=32, trim=False, runs=((True, 0), (False, 0), (True, 1))):
    """{(pack, k): (loss, logits, flat grads, ctx grad)} of one forward_backward per run, all with the same seed."""
    import lora_train_vlp as L
    from clipfs import synth
    sd_ctx = model.token_embedding.weight.data[[5, 6, 7, 8]].clone()
    ctx = torch.nn.Parameter(sd_ctx) if with_ctx else None
    tr = L.LoRATrainer(model, prompt_ctx=ctx, shard_text=False)
    img = synth.synth_images(n_img, cfg.image_resolution, seed=0).to(dev)
    cap = cap.to(dev)
    tgt = synth.synth_labels(n_img, cap.shape[0], seed=2).to(dev)
    eng = model.engine
    eng.trim_text = trim
    out = {}
    for pack, k in runs:
        eng.pack_text_backward = pack
        eng.step = 3
        tr.flat.zero_grad()
        loss, _, logits = tr.forward_backward(img, cap, tgt)
        torch.cuda.synchronize()
        out[(pack, k)] = (loss.clone(), logits.clone(), tr.flat.grads.clone())
    return out, tr


def _packs(model, tr, cap, trim=False):
    """Whether the text backward of these runs took the packed rows (the library's own decision for this geometry)."""
    eng = model.engine
    eng.trim_text = trim
    ids, seq = eng._effective_ids(cap.to(model.device).contiguous())
    plan, R = eng._pack_plan(ids)
    lo = tr.last_plan["text"]
    return eng.txt.pack_mode(ids.shape[0], R, 1, seq, lo)


def _check(out, tr):
    lp, gp = out[(True, 0)][1], out[(True, 0)][2]
    ld, gd = out[(False, 0)][1], out[(False, 0)][2]
    assert torch.equal(out[(True, 0)][0], out[(False, 0)][0])
    assert torch.equal(lp, ld)
    # every trainable tensor within REL of its own largest magnitude
    scale_all = gd.abs().max().item()
    assert scale_all > 0
    for name, view_p, view_d in _views(tr, gp, gd):
        scale = view_d.abs().max().item()
        err = (view_p - view_d).abs().max().item()
        # a gradient that is zero up to rounding (the key bias: softmax is shift-invariant) has no scale of its own:
        # its budget is taken from 1e-3 of the largest gradient
        assert err <= REL * max(scale, 1e-3 * scale_all), (name, err, scale, scale_all)
    if (True, 1) in out:
        assert torch.equal(out[(True, 1)][1], lp)
        assert torch.equal(out[(True, 1)][2], gp)


def _views(tr, gp, gd):
    """(name, slice of packed grads, slice of dense grads) per trainable of the flat buffer."""
    off, res = 0, []
    for i, n in enumerate(_numels(tr)):
        res.append((str(i), gp[off:off + n], gd[off:off + n]))
        off += n
    assert off == gp.numel()
    return res


def _numels(tr):
    """sizes of the trainables in flat-buffer order: cut at every tensor that is a view of the flat parameters"""
    f = tr.flat
    base, n = f.params.data_ptr(), f.params.numel()
    starts = {0}
    tensors = [p for p in tr.model.parameters()] + ([tr.prompt_ctx] if tr.prompt_ctx is not None else [])
    for mod in tr.model.modules():
        if hasattr(mod, "stacked") and getattr(mod, "is_lora_mha", False):
            tensors += [p for _, p, _ in mod.stacked()]
    for t in tensors:
        o = (t.data_ptr() - base) // 4
        if 0 <= o < n:
            starts.add(o)
    cuts = sorted(starts) + [n]
    return [b - a for a, b in zip(cuts[:-1], cuts[1:])]


def _bench_caps(cfg):
    from clipfs import synth
    return synth.synth_captions(403, 77, cfg.vocab_size, seed=1)


def test_plan_matches_the_captions(dev):
    from clipfs import ops
    model, cfg = _model(dev)
    cap = _bench_caps(cfg).to(dev)
    plan, R = model.engine._pack_plan(cap)
    eot = ops.eot_index(cap).long().cpu()
    assert R == int((eot + 1).sum()) == 9748
    n, seq = cap.shape
    pl = plan.long().cpu()
    off, eotp, rows = pl[:n + 1], pl[n + 1:2 * n + 1], pl[2 * n + 1:]
    assert off[0] == 0 and off[-1] == R and torch.equal(eotp, off[1:] - 1)
    want = torch.cat([c * seq + torch.arange(int(eot[c]) + 1) for c in range(n)])
    assert torch.equal(rows, want)
    assert model.engine.txt.pack_mode(n, R, seed=1, seq=seq)


def test_cfg2_geometry_ctx_bias_all(dev):
    """403 x 77 captions of the bench, dropout 0.25, prompt ctx, bias='all'."""
    model, cfg = _model(dev, bias="all")
    out, tr = _run(dev, model, cfg, _bench_caps(cfg))
    assert _packs(model, tr, _bench_caps(cfg))
    _check(out, tr)


@pytest.mark.parametrize("case", ["full_and_shortest", "fallback_long", "trim_text"])
def test_edge_tables(dev, case):
    model, cfg = _model(dev)
    if case == "full_and_shortest":  # EOT at 76, the shortest caption (SOT, EOT), the rest short
        lens = [77, 2, 3] + [int(x) for x in np.random.RandomState(3).randint(2, 20, size=37)]
        cap = _captions(lens)
    elif case == "fallback_long":  # R > M / 2: the dense rows, bitwise as before
        cap = _captions([int(x) for x in np.random.RandomState(4).randint(50, 78, size=40)])
    else:  # one 50-token caption among short ones: trimmed to seq 50 (4 attention tiles), R well under M / 2
        lens = [50] + [int(x) for x in np.random.RandomState(5).randint(3, 11, size=99)]
        cap = _captions(lens)
    trim = case == "trim_text"
    out, tr = _run(dev, model, cfg, cap, trim=trim)
    assert _packs(model, tr, cap, trim) == (case != "fallback_long")
    if trim:
        assert model.engine._effective_ids(cap.to(dev))[1] == 50
    _check(out, tr)
    if case == "fallback_long":
        assert torch.equal(out[(True, 0)][2], out[(False, 0)][2])


def test_text_up_floor(dev):
    model, cfg = _model(dev, position="up")
    out, tr = _run(dev, model, cfg, _bench_caps(cfg)[:96], with_ctx=False)
    assert tr.last_plan["text"] == 8
    assert _packs(model, tr, _bench_caps(cfg)[:96])
    _check(out, tr)


def test_frozen_text_adapters(dev):
    model, cfg = _model(dev, freeze_text=True)
    out, tr = _run(dev, model, cfg, _bench_caps(cfg)[:96])
    assert tr.last_plan["text"] == 0
    assert _packs(model, tr, _bench_caps(cfg)[:96])
    _check(out, tr)


@pytest.mark.parametrize("seq,L", [(77, 2), (77, 7), (77, 16), (77, 17), (77, 40), (77, 77), (41, 41), (41, 9),
                                   (20, 20), (20, 3), (96, 96), (96, 50), (16, 16)])
def test_packed_attention_against_fp64(dev, seq, L):
    """clipfs_attention_bwd_packed for captions of length L (and a mix) in sequences of `seq` tokens (1 ... 6 tiles: the
    trimmed text tower runs seq < 77) against fp64 autograd of the oracle's sdpa, and bitwise against the full-layout
    kernel given the same dO with zero dead rows."""
    from clipfs import _lib
    from oracle import clip_oracle as O
    lib = _lib.load()
    B, H = 5, 8
    d = 64 * H
    lens = torch.tensor([L, max(1, L // 2), 1, L, min(seq, L + 3)], dtype=torch.int64)
    g = torch.Generator().manual_seed(100 * seq + L)
    qkv = torch.randn(B * seq, 3 * d, generator=g)
    dout_full = torch.randn(B * seq, d, generator=g)
    live = (torch.arange(seq)[None, :] < lens[:, None]).reshape(-1)
    dout_full[~live] = 0
    mask = O.build_causal_mask(seq, torch.float64)
    q, k, v = (qkv.double().reshape(B, seq, 3, H, 64).permute(2, 0, 3, 1, 4)[i].clone().requires_grad_() for i in range(3))
    o = O.sdpa(q, k, v, mask)
    o.backward(dout_full.double().reshape(B, seq, H, 64).permute(0, 2, 1, 3))
    ref = torch.cat([t.grad.permute(0, 2, 1, 3).reshape(B * seq, d) for t in (q, k, v)], 1)
    out = o.detach().permute(0, 2, 1, 3).reshape(B * seq, d).float()
    # lse from fp64: the forward kernel's statistic, log-sum-exp of the scaled scores per (b, h, query)
    s = (q @ k.transpose(-2, -1)) / 8.0 + mask
    lse = torch.logsumexp(s, -1).detach().float().reshape(-1)
    off = torch.zeros(B + 1, dtype=torch.int32)
    off[1:] = torch.cumsum(lens, 0).to(torch.int32)
    R = int(off[-1])
    dq = qkv.to(dev), out.to(dev), lse.to(dev)
    dout_p = dout_full[live].contiguous().to(dev)
    dqkv_p = torch.full((R, 3 * d), float("nan"), device=dev)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.clipfs_attention_bwd_packed(dq[0].data_ptr(), dout_p.data_ptr(), dq[1].data_ptr(), dq[2].data_ptr(),
                                           dqkv_p.data_ptr(), off.to(dev).data_ptr(), B, seq, H, st) == 0
    dqkv_f = torch.zeros(B * seq, 3 * d, device=dev)
    work = torch.empty(B * H * seq, device=dev)
    dfull = dout_full.to(dev)
    assert lib.clipfs_attention_bwd(dq[0].data_ptr(), dfull.data_ptr(), dq[1].data_ptr(), dq[2].data_ptr(),
                                    dqkv_f.data_ptr(), work.data_ptr(), B, seq, H, 1, st) == 0
    torch.cuda.synchronize()
    got = dqkv_p.cpu()
    assert torch.isfinite(got).all()
    want = ref[live]
    err = (got.double() - want).abs().max().item()
    assert err <= 1e-4 * want.abs().max().item(), err
    assert torch.equal(got, dqkv_f.cpu()[live])


# ---- two class-sharded ranks ---------------------------------------------------------------------------------------
def _free_port():
    import socket
    so = socket.socket()
    so.bind(("127.0.0.1", 0))
    port = so.getsockname()[1]
    so.close()
    return port


def _rank_main(rank, world, port, out_dir):
    """One rank of a 2-rank class-sharded step (65 captions x 77 = 5 005 text rows per rank), packed and all-rows."""
    import os
    import sys
    import torch.distributed as dist
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for path in (os.path.join(root, "jittor-clip-fewshot_amd"), root):
        if path not in sys.path:
            sys.path.insert(0, path)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import lora_train_vlp as L
    from clipfs import dist as D
    from clipfs import synth
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda:0")
    model, cfg = _model(dev)
    ctx = torch.nn.Parameter(model.token_embedding.weight.data[[5, 6, 7, 8]].clone())
    tr = L.LoRATrainer(model, prompt_ctx=ctx, shard_text=True)
    cap = _bench_caps(cfg)[:130].to(dev)
    img = synth.synth_images(8, cfg.image_resolution, seed=0).to(dev)
    tgt = synth.synth_labels(8, 130, seed=2).to(dev)
    lo, hi = D.shard_bounds(8, rank, world)
    c_lo, c_hi = D.block_bounds(130, rank, world)
    block = cap[c_lo:c_hi].contiguous()
    eng = model.engine
    res = {}
    for pack in (True, False):
        eng.pack_text_backward = pack
        eng.step = 3
        tr.flat.zero_grad()
        loss, _, logits = tr.forward_backward(img[lo:hi].contiguous(), cap, tgt[lo:hi].contiguous(), 1, 8, row_offset=lo)
        torch.cuda.synchronize()
        res[pack] = (loss.cpu().numpy(), logits.cpu().numpy(), tr.flat.grads.cpu().numpy())
    plan, R = eng._pack_plan(block)
    packs = eng.txt.pack_mode(block.shape[0], R, 1, 77, tr.last_plan["text"])
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), loss_p=res[True][0], loss_d=res[False][0], logits_p=res[True][1],
             logits_d=res[False][1], g_p=res[True][2], g_d=res[False][2], packs=np.array(packs), rows=np.array(block.numel()))
    dist.destroy_process_group()


def test_two_class_sharded_ranks(tmp_path):
    """shard_text with two ranks: each rank's caption block (65 x 77 rows, dropout rows offset by the block) packs, and
    matches the all-rows backward of the same step (loss and logits bitwise, gradients within the fp32 reorder budget)."""
    import os
    import torch.multiprocessing as mp
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    mp.spawn(_rank_main, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    for rank in (0, 1):
        z = np.load(os.path.join(str(tmp_path), f"rank{rank}.npz"))
        assert bool(z["packs"]) and int(z["rows"]) >= 2048
        assert np.array_equal(z["loss_p"], z["loss_d"]) and np.array_equal(z["logits_p"], z["logits_d"])
        scale = np.abs(z["g_d"]).max()
        assert scale > 0
        assert np.abs(z["g_p"] - z["g_d"]).max() <= REL * scale
