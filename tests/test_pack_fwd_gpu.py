"""Live-row text forward (clipfs_tower_fwd_packed, Engine.pack_text_forward) against the dense forward.

Every live row of every block is computed from the same values in the same order as in the dense forward, so features,
saved activations (dropout keep bits included), loss, logits and gradients are bitwise equal."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAMES = {"q": "q_proj", "k": "k_proj", "v": "v_proj"}


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


def _model(dev, position="all", bias="none", p=0.25):
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
    model.train()
    return model, cfg


def _bench_caps(cfg):
    from clipfs import synth
    return synth.synth_captions(403, 77, cfg.vocab_size, seed=1)


def _table(cfg, name):
    rs = np.random.RandomState(11)
    if name == "bench":
        return _bench_caps(cfg)
    if name == "eot1":  # every EOT at position 1: one 16-token tile, two live rows per caption
        return _captions([2] * 60)
    if name == "tile_edges":  # EOT at 15 / 16 / 17: the last live token at a tile's end, a tile's start, one past it
        return _captions([16, 17, 18] * 20)
    if name == "mixed":
        return _captions([77, 2, 33] + [int(v) for v in rs.randint(2, 30, size=57)])
    return _captions([int(v) for v in rs.randint(50, 78, size=40)])  # "fallback": R > M / 2


# ---- saved layout (tower.hip saved_layout_rows, exact fp32 mode) -----------------------------------------------------
def _al4(n):
    return (n + 3) & ~3


def _layout(lib, rows, batch, seq, d, heads, r, keep):
    o, L = 0, {}
    for name, n in (("x_in", rows * d), ("stat1", 2 * rows), ("h1", rows * d), ("t_qkv", rows * 3 * r), ("qkv", rows * 3 * d),
                    ("att", rows * d), ("lse", lib.clipfs_attention_lse_floats(batch, seq, heads)), ("t_o", rows * r),
                    ("x_mid", rows * d), ("stat2", 2 * rows), ("u", rows * 4 * d),
                    ("keep", (rows * (d // 4) + 1) // 2 if keep else 0)):
        L[name] = o
        o += _al4(n)
    L["total"] = o
    return L


def _rowwise(rec, L, name, rows, w):
    return rec[L[name]:L[name] + rows * w].view(rows, w)


def _keep(rec, L, rows, d):
    return rec[L["keep"]:L["keep"] + _al4((rows * (d // 4) + 1) // 2)].view(torch.int16)[:rows * (d // 4)].view(rows, d // 4)


@pytest.mark.parametrize("table", ["bench", "eot1", "tile_edges", "mixed", "fallback"])
def test_tower_forward_against_rows(dev, table):
    """clipfs_tower_fwd_packed against clipfs_tower_fwd_rows: 12 blocks of width 512, dropout 0.25, a non-zero seed and
    the dropout rows of a class-sharded rank (row0 = 7 captions): the EOT output rows and every saved tensor bitwise."""
    from clipfs import _lib, ops
    lib = _lib.load()
    model, cfg = _model(dev)
    eng, txt = model.engine, model.engine.txt
    ids = _table(cfg, table).to(dev)
    n, seq = ids.shape
    d, H, M = txt.width, txt.heads, n * seq
    x0 = ops.text_embed(ids, model.token_embedding.weight.data, model.positional_embedding.data, None)
    eot = ops.eot_index(ids)
    plan, R = eng._pack_plan(ids)
    seed, row0 = 0x1234567, 7
    packs = txt.pack_fwd_mode(n, R, seed, seq, 0)
    assert packs == (table != "fallback")
    xd, xp = x0.clone(), x0.clone()
    sd = txt.forward(xd, n, True, seed, seq, own_saved=True, row0=row0, rows=eot, grad_lo=0)
    sp = txt.forward(xp, n, True, seed, seq, own_saved=True, row0=row0, rows=eot, grad_lo=0, pack=(plan, R))
    torch.cuda.synchronize()
    assert sp.numel() == sd.numel()
    ar = torch.arange(n, device=dev)
    el = eot.long()
    assert torch.equal(xp.view(n, seq, d)[ar, el], xd.view(n, seq, d)[ar, el])
    r = txt.lora_r
    Ld = _layout(lib, M, n, seq, d, H, r, True)
    eotf = ar * seq + el
    lens = (el + 1).cpu()
    live = (torch.arange(seq)[None, :] < lens[:, None])  # [n, seq]
    if packs:
        Lp, mp, eotp = _layout(lib, R, n, seq, d, H, r, True), plan[2 * n + 1:].long(), plan[n + 1:2 * n + 1].long()
    else:  # the dense forward, in its own layout (what it writes: rows it skips stay uninitialised in both buffers)
        Lp, mp, eotp, R = Ld, torch.arange(M, device=dev), eotf, M
        live = torch.ones(n, seq, dtype=torch.bool)
    for l in range(txt.layers):
        rd = sd[l * Ld["total"]:(l + 1) * Ld["total"]]
        rp = sp[l * Lp["total"]:(l + 1) * Lp["total"]]
        last = l == txt.layers - 1
        for name, w in (("x_in", d), ("h1", d), ("t_qkv", 3 * r), ("qkv", 3 * d), ("att", d)):
            assert torch.equal(_rowwise(rp, Lp, name, R, w), _rowwise(rd, Ld, name, M, w)[mp]), (l, name)
        for k in range(2):  # mean, rstd
            assert torch.equal(rp[Lp["stat1"] + k * R:Lp["stat1"] + (k + 1) * R],
                               rd[Ld["stat1"] + k * M:Ld["stat1"] + (k + 1) * M][mp]), (l, "stat1", k)
        assert torch.equal(_keep(rp, Lp, R, d), _keep(rd, Ld, M, d)[mp]), (l, "keep")
        lse_d = rd[Ld["lse"]:Ld["lse"] + n * H * seq].view(n, H, seq).cpu()
        lse_p = rp[Lp["lse"]:Lp["lse"] + n * H * seq].view(n, H, seq).cpu()
        lm = live[:, None, :].expand(n, H, seq)
        assert torch.equal(lse_p[lm], lse_d[lm]), (l, "lse")
        sel_p, sel_d = (eotp, eotf) if last else (torch.arange(R, device=dev), mp)
        for name, w in (("x_mid", d), ("u", 4 * d)):
            assert torch.equal(_rowwise(rp, Lp, name, R, w)[sel_p], _rowwise(rd, Ld, name, M, w)[sel_d]), (l, name)
        for k in range(2):
            assert torch.equal(rp[Lp["stat2"] + k * R:Lp["stat2"] + (k + 1) * R][sel_p],
                               rd[Ld["stat2"] + k * M:Ld["stat2"] + (k + 1) * M][sel_d]), (l, "stat2", k)


@pytest.mark.parametrize("seq,L", [(77, 2), (77, 16), (77, 17), (77, 40), (77, 77), (41, 9), (20, 20), (96, 50),
                                   (16, 16)])
def test_packed_attention_forward(dev, seq, L):
    """clipfs_attention_fwd_packed against the full-layout kernel (bitwise on live rows and live lse entries) and fp64
    sdpa; clipfs_attention_bwd_packed_io on those packed tensors against clipfs_attention_bwd_packed on the full ones."""
    from clipfs import _lib
    from oracle import clip_oracle as O
    lib = _lib.load()
    B, H = 5, 8
    d = 64 * H
    lens = torch.tensor([L, max(1, L // 2), 1, L, min(seq, L + 3)], dtype=torch.int64)
    g = torch.Generator().manual_seed(7 * seq + L)
    qkv = torch.randn(B * seq, 3 * d, generator=g)
    live = (torch.arange(seq)[None, :] < lens[:, None]).reshape(-1)
    off = torch.zeros(B + 1, dtype=torch.int32)
    off[1:] = torch.cumsum(lens, 0).to(torch.int32)
    R = int(off[-1])
    st = torch.cuda.current_stream().cuda_stream
    qf, qp, offd = qkv.to(dev), qkv[live].contiguous().to(dev), off.to(dev)
    out_f = torch.zeros(B * seq, d, device=dev)
    lse_f = torch.zeros(B * H * seq, device=dev)
    out_p = torch.full((R, d), float("nan"), device=dev)
    lse_p = torch.full((B * H * seq,), float("nan"), device=dev)
    assert lib.clipfs_attention_fwd(qf.data_ptr(), out_f.data_ptr(), lse_f.data_ptr(), B, seq, H, 1, st) == 0
    assert lib.clipfs_attention_fwd_packed(qp.data_ptr(), out_p.data_ptr(), lse_p.data_ptr(), offd.data_ptr(), B, seq, H,
                                           st) == 0
    torch.cuda.synchronize()
    assert torch.equal(out_p.cpu(), out_f.cpu()[live])
    lm = live.view(B, 1, seq).expand(B, H, seq).reshape(-1)
    assert torch.equal(lse_p.cpu()[lm], lse_f.cpu()[lm])
    mask = O.build_causal_mask(seq, torch.float64)
    q, k, v = (qkv.double().reshape(B, seq, 3, H, 64).permute(2, 0, 3, 1, 4)[i] for i in range(3))
    ref = O.sdpa(q, k, v, mask).permute(0, 2, 1, 3).reshape(B * seq, d)[live]
    err = (out_p.cpu().double() - ref).abs().max().item()
    assert err <= 1e-5 * ref.abs().max().item(), err
    # backward over the packed tensors: bitwise the backward over the full-layout ones
    dout = torch.randn(R, d, generator=g).to(dev)
    dq_a = torch.full((R, 3 * d), float("nan"), device=dev)
    dq_b = torch.full((R, 3 * d), float("nan"), device=dev)
    assert lib.clipfs_attention_bwd_packed(qf.data_ptr(), dout.data_ptr(), out_f.data_ptr(), lse_f.data_ptr(), dq_a.data_ptr(),
                                           offd.data_ptr(), B, seq, H, st) == 0
    assert lib.clipfs_attention_bwd_packed_io(qp.data_ptr(), dout.data_ptr(), out_p.data_ptr(), lse_p.data_ptr(),
                                              dq_b.data_ptr(), offd.data_ptr(), B, seq, H, st) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(dq_b).all()
    assert torch.equal(dq_a, dq_b)


# ---- training steps ---------------------------------------------------------------------------------------------------
def _run(dev, model, cfg, cap, with_ctx=True, n_img=32):
    """{pack_text_forward: (loss, logits, flat grads)} of one forward_backward each, same seed."""
    import lora_train_vlp as L
    from clipfs import synth
    ctx = torch.nn.Parameter(model.token_embedding.weight.data[[5, 6, 7, 8]].clone()) if with_ctx else None
    tr = L.LoRATrainer(model, prompt_ctx=ctx, shard_text=False)
    img = synth.synth_images(n_img, cfg.image_resolution, seed=0).to(dev)
    cap = cap.to(dev)
    tgt = synth.synth_labels(n_img, cap.shape[0], seed=2).to(dev)
    eng = model.engine
    out = {}
    for fwd in (True, False):
        eng.pack_text_forward = fwd
        eng.step = 3
        tr.flat.zero_grad()
        loss, _, logits = tr.forward_backward(img, cap, tgt)
        torch.cuda.synchronize()
        out[fwd] = (loss.clone(), logits.clone(), tr.flat.grads.clone())
    eng.pack_text_forward = True
    return out, tr


def _packs_fwd(model, tr, cap):
    eng = model.engine
    ids = cap.to(model.device).contiguous()
    plan, R = eng._pack_plan(ids)
    return eng.txt.pack_fwd_mode(ids.shape[0], R, 1, ids.shape[1], tr.last_plan["text"])


@pytest.mark.parametrize("case", ["ctx_bias_all", "text_up_floor"])
def test_training_step(dev, case):
    """forward_backward with and without the live-row forward: loss, logits and every gradient bitwise."""
    if case == "ctx_bias_all":
        model, cfg = _model(dev, bias="all")
        cap, with_ctx = _bench_caps(cfg), True
    else:
        model, cfg = _model(dev, position="up")
        cap, with_ctx = _bench_caps(cfg)[:96], False
    out, tr = _run(dev, model, cfg, cap, with_ctx)
    if case == "text_up_floor":
        assert tr.last_plan["text"] == 8
    assert _packs_fwd(model, tr, cap)
    assert torch.equal(out[True][0], out[False][0])
    assert torch.equal(out[True][1], out[False][1])
    assert torch.equal(out[True][2], out[False][2])


def test_no_grad_features(dev):
    """the no-grad text forward (classifier build, eval) takes the live rows too: features bitwise, with and without
    dropout (train mode with a seed)."""
    model, cfg = _model(dev)
    eng = model.engine
    ids = _bench_caps(cfg).to(dev)
    plan, R = eng._pack_plan(ids)
    assert eng.txt.pack_fwd_mode(ids.shape[0], R, 99, 77, 0, train=False)
    res = {}
    for fwd in (True, False):
        eng.pack_text_forward = fwd
        model.train()
        f_drop, _ = eng.text_forward(ids, None, False, seed=99)
        model.eval()
        f_eval, _ = eng.text_forward(ids, None, False, seed=0)
        torch.cuda.synchronize()
        res[fwd] = (f_drop.clone(), f_eval.clone())
    eng.pack_text_forward = True
    assert torch.equal(res[True][0], res[False][0])
    assert torch.equal(res[True][1], res[False][1])
    assert not torch.equal(res[True][0], res[True][1])  # dropout did act


def test_fallbacks(dev):
    """pack_text_backward = False, trim_text at the bench table, the fp16 storage mode and small towers: dense forward."""
    model, cfg = _model(dev)
    eng = model.engine
    ids = _bench_caps(cfg).to(dev)
    _, ctx = eng.text_forward(ids, None, True, seed=5)
    assert ctx["pack"] is not None and ctx["pack_fwd"]
    eng.pack_text_backward = False
    _, ctx = eng.text_forward(ids, None, True, seed=5)
    assert ctx["pack"] is None and not ctx["pack_fwd"]
    eng.pack_text_backward = True
    eng.trim_text = True
    _, ctx = eng.text_forward(ids, None, True, seed=5)
    assert not ctx["pack_fwd"]
    eng.trim_text = False
    _, ctx = eng.text_forward(ids[:20], None, True, seed=5)  # 1540 rows
    assert not ctx["pack_fwd"]
    plan, R = eng._pack_plan(ids)
    eng.precision = "fp16"
    try:
        assert not eng.txt.pack_fwd_mode(ids.shape[0], R, 5, 77, 0)
    finally:
        eng.precision = "fp32"
    torch.cuda.synchronize()


# ---- two class-sharded ranks ---------------------------------------------------------------------------------------
def _free_port():
    import socket
    so = socket.socket()
    so.bind(("127.0.0.1", 0))
    port = so.getsockname()[1]
    so.close()
    return port


def _rank_main(rank, world, port, out_dir):
    """One rank of a 2-rank class-sharded step (65 captions x 77 = 5 005 text rows per rank, dropout rows offset by the
    rank's caption block), with and without the live-row forward."""
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
    for fwd in (True, False):
        eng.pack_text_forward = fwd
        eng.step = 3
        tr.flat.zero_grad()
        loss, _, logits = tr.forward_backward(img[lo:hi].contiguous(), cap, tgt[lo:hi].contiguous(), 1, 8, row_offset=lo)
        torch.cuda.synchronize()
        res[fwd] = (loss.cpu().numpy(), logits.cpu().numpy(), tr.flat.grads.cpu().numpy())
    plan, R = eng._pack_plan(block)
    packs = eng.txt.pack_fwd_mode(block.shape[0], R, 1, 77, tr.last_plan["text"])
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), loss_p=res[True][0], loss_d=res[False][0], logits_p=res[True][1],
             logits_d=res[False][1], g_p=res[True][2], g_d=res[False][2], packs=np.array(packs))
    dist.destroy_process_group()


def test_two_class_sharded_ranks_forward(tmp_path):
    import os
    import torch.multiprocessing as mp
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    mp.spawn(_rank_main, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    for rank in (0, 1):
        z = np.load(os.path.join(str(tmp_path), f"rank{rank}.npz"))
        assert bool(z["packs"])
        assert np.array_equal(z["loss_p"], z["loss_d"]) and np.array_equal(z["logits_p"], z["logits_d"])
        assert np.array_equal(z["g_p"], z["g_d"])
