"""Workspace independence at the kernel level: every entry point that takes caller scratch, or writes into freshly
allocated outputs, runs three times on the same seeded inputs with all that memory pre-filled with 0.0, NaN and 1e30
(tests/poison.py).  The documented outputs must agree bit for bit across the fills and be finite; buffers sized by an
exact query carry a 64-float tail that must keep its fill; regions the header documents as unwritten or exact zero must
hold what it says.  Accumulating outputs (dA / dB / dx of clipfs_lora_bwd*, the bias gradient slots) are pre-filled with
seeded finite values in every run: they accumulate by contract.

Nothing here compares against a reference: the sibling parity tests do (test_kernels_gpu.py, test_edge_cases_gpu.py,
test_lora_rank_gpu.py, test_glue_kernels_gpu.py ...).  A kernel that reads a slot before writing it, relies on an earlier
call's leftovers or multiplies a masked 0 with a stale row passes those on clean memory and fails here.
tests/workspace_cases.py maps every entry point of include/clipfs.h with such a parameter to its test below."""
import pytest
import torch

from poison import FILLS, assert_same_runs, fill_value, poisoned, same_bits

pytestmark = pytest.mark.gpu

TAIL = 64


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _randn(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _buf(n, fill, dev, dtype=torch.float32):
    """An explicitly poisoned buffer of ``n`` elements."""
    return torch.full((int(n),), fill_value(dtype, fill), device=dev, dtype=dtype)


def _keeps(t, fill):
    """Whether every element of ``t`` still holds ``fill``, bit for bit."""
    return same_bits(t, torch.full_like(t, fill_value(t.dtype, fill)))


# ------------------------------------------------------------------------------------------------ fp32 attention
# (batch, seq, heads, causal, family of the forward and of the backward with statistics)
ATTN = [(2, 50, 2, True, "mfma16"), (3, 77, 2, True, "mfma16"), (1, 130, 2, False, "mfma32"),
        (1, 289, 1, True, "mfma_long"), (1, 1025, 1, True, "stream")]


def _attn_run(lib, dev, fill, qkv, dout, B, L, H, causal, stats, misalign=0):
    """Forward + backward with every buffer passed by this test: out / dqkv poisoned, lse / work sized to
    clipfs_attention_lse_floats plus a tail.  ``misalign``: floats by which out and dqkv are off 16-byte alignment."""
    d = 64 * H
    n = lib.clipfs_attention_lse_floats(B, L, H)
    assert n == B * H * L
    out_b = _buf(B * L * d + misalign + TAIL, fill, dev)
    dq_b = _buf(B * L * 3 * d + misalign + TAIL, fill, dev)
    out = out_b[misalign:misalign + B * L * d]
    dqkv = dq_b[misalign:misalign + B * L * 3 * d]
    lse = _buf(n + TAIL, fill, dev) if stats else None
    work = _buf(n + TAIL, fill, dev) if stats else None
    p = lambda t: None if t is None else t.data_ptr()
    assert lib.clipfs_attention_fwd(qkv.data_ptr(), out.data_ptr(), p(lse), B, L, H, int(causal), _st()) == 0
    if stats or L <= 96:
        assert lib.clipfs_attention_bwd(qkv.data_ptr(), dout.data_ptr(), out.data_ptr() if stats else None, p(lse),
                                        dqkv.data_ptr(), p(work), B, L, H, int(causal), _st()) == 0
    else:
        dqkv = None  # a backward without statistics is refused past 96 tokens: forward only
    torch.cuda.synchronize()
    res = {"out": out.clone()}
    if dqkv is not None:
        res["dqkv"] = dqkv.clone()
        assert _keeps(dq_b[:misalign], fill) and _keeps(dq_b[misalign + B * L * 3 * d:], fill), "dqkv: written outside"
    assert _keeps(out_b[:misalign], fill) and _keeps(out_b[misalign + B * L * d:], fill), "out: written outside"
    if stats:
        res["lse"] = lse[:n].clone()
        assert _keeps(lse[n:], fill), "lse: tail written"
        assert _keeps(work[n:], fill), "work: tail written"
    return res


@pytest.mark.parametrize("stats", [True, False], ids=["stats", "nostats"])
@pytest.mark.parametrize("B,L,H,causal,family", ATTN)
def test_attention_fp32(dev, B, L, H, causal, family, stats):
    from clipfs import _lib
    lib = _lib.load()
    assert _lib.attention_plan("fwd", B, L, H, causal, stats=stats)["family"] == family
    if stats:
        assert _lib.attention_plan("bwd", B, L, H, causal)["family"] == family
    elif L <= 96:
        assert _lib.attention_plan("bwd", B, L, H, causal, stats=False)["family"] == "recompute"
    qkv = _randn(B * L, 3 * 64 * H, seed=100 + L).to(dev)
    dout = _randn(B * L, 64 * H, seed=200 + L).to(dev)
    assert_same_runs([_attn_run(lib, dev, f, qkv, dout, B, L, H, causal, stats) for f in FILLS])


def test_attention_fp32_recompute_65(dev):
    """(2, 65, 1) without statistics: the lmax = 80 instance of the softmax-recomputing backward."""
    from clipfs import _lib
    lib = _lib.load()
    plan = _lib.attention_plan("bwd", 2, 65, 1, True, stats=False)
    assert plan["family"] == "recompute" and plan["lmax"] == 80
    qkv = _randn(2 * 65, 192, seed=1).to(dev)
    dout = _randn(2 * 65, 64, seed=2).to(dev)
    assert_same_runs([_attn_run(lib, dev, f, qkv, dout, 2, 65, 1, True, False) for f in FILLS])


def test_attention_fp32_misaligned_streams(dev):
    """out / dqkv one float off 16-byte alignment: the streaming kernels at a length the MFMA kernels own otherwise."""
    from clipfs import _lib
    lib = _lib.load()
    for direction in ("fwd", "bwd"):
        assert _lib.attention_plan(direction, 2, 50, 2, True, aligned=False)["family"] == "stream"
    qkv = _randn(100, 384, seed=3).to(dev)
    dout = _randn(100, 128, seed=4).to(dev)
    assert_same_runs([_attn_run(lib, dev, f, qkv, dout, 2, 50, 2, True, True, misalign=1) for f in FILLS])


# ------------------------------------------------------------------------------------------------ packed attention
PACK_LENS = [77, 2, 16, 17, 33, 2]  # the last caption is short: the packed buffers end right after a 2-row sequence
GUARD = 80                          # poisoned rows behind off[batch], inside the allocation


def _pack_off(dev):
    lens = torch.tensor(PACK_LENS, dtype=torch.int64)
    off = torch.zeros(len(PACK_LENS) + 1, dtype=torch.int32)
    off[1:] = torch.cumsum(lens, 0).to(torch.int32)
    live = torch.arange(77)[None, :] < lens[:, None]
    return off.to(dev), int(off[-1]), live


def _guarded(rows, fill, dev, dtype=torch.float32):
    """``rows`` [R, w] followed by GUARD rows of ``fill`` in one allocation; returns (whole buffer, its first R rows)."""
    R, w = rows.shape
    whole = torch.full((R + GUARD, w), fill_value(dtype, fill), device=dev, dtype=dtype)
    whole[:R] = rows.to(device=dev, dtype=dtype)
    return whole, whole[:R]


def test_attention_packed(dev):
    """clipfs_attention_fwd_packed, _bwd_packed (dense records) and _bwd_packed_io (packed records): every packed tensor
    is allocated at exactly off[batch] rows and followed by poisoned guard rows, which a clamped or masked read of "rows
    past the end" would pull into a live row.  lse entries past Lb are documented unwritten."""
    from clipfs import _lib
    lib = _lib.load()
    B, L, H = len(PACK_LENS), 77, 2
    d = 64 * H
    assert lib.clipfs_attention_bwd_packed_ok(L, 1)
    assert _lib.attention_plan("fwd_packed", B, L, H, True)["family"] == "mfma16_packed"
    assert _lib.attention_plan("bwd_packed", B, L, H, True)["family"] == "mfma16_packed"
    assert _lib.attention_plan("bwd_packed_io", B, L, H, True)["family"] == "mfma16_pinned"
    off, R, live = _pack_off(dev)
    qkv_full = _randn(B * L, 3 * d, seed=11)
    dout_p = _randn(R, d, seed=12)
    qf = qkv_full.to(dev)
    nl = lib.clipfs_attention_lse_floats(B, L, H)
    # the dense forward's records, for clipfs_attention_bwd_packed
    out_f = torch.zeros(B * L, d, device=dev)
    lse_f = torch.zeros(nl, device=dev)
    assert lib.clipfs_attention_fwd(qf.data_ptr(), out_f.data_ptr(), lse_f.data_ptr(), B, L, H, 1, _st()) == 0
    lm = live.view(B, 1, L).expand(B, H, L).reshape(-1).to(dev)
    runs = []
    for fill in FILLS:
        qp_all, qp = _guarded(qkv_full[live.reshape(-1)], fill, dev)
        dp_all, dp = _guarded(dout_p, fill, dev)
        out_all, out = _guarded(torch.zeros(R, d), fill, dev)
        out.fill_(fill)
        lse = _buf(nl + TAIL, fill, dev)
        assert lib.clipfs_attention_fwd_packed(qp.data_ptr(), out.data_ptr(), lse.data_ptr(), off.data_ptr(), B, L, H, _st()) == 0
        dq = {}
        for name in ("dense", "io"):
            dq_all, dq[name] = _guarded(torch.zeros(R, 3 * d), fill, dev)
            dq[name].fill_(fill)
            dq[name + "_all"] = dq_all
        assert lib.clipfs_attention_bwd_packed(qf.data_ptr(), dp.data_ptr(), out_f.data_ptr(), lse_f.data_ptr(),
                                               dq["dense"].data_ptr(), off.data_ptr(), B, L, H, _st()) == 0
        assert lib.clipfs_attention_bwd_packed_io(qp.data_ptr(), dp.data_ptr(), out.data_ptr(), lse.data_ptr(),
                                                  dq["io"].data_ptr(), off.data_ptr(), B, L, H, _st()) == 0
        torch.cuda.synchronize()
        assert _keeps(out_all[R:], fill), "out: guard rows written"
        assert _keeps(dq["dense_all"][R:], fill) and _keeps(dq["io_all"][R:], fill), "dqkv: guard rows written"
        assert _keeps(lse[nl:], fill), "lse: tail written"
        assert _keeps(lse[:nl][~lm], fill), "lse: entries past Lb are documented unwritten"
        runs.append({"out": out.clone(), "lse_live": lse[:nl][lm].clone(), "dqkv_dense": dq["dense"].clone(),
                     "dqkv_io": dq["io"].clone()})
    assert_same_runs(runs)
    assert same_bits(runs[0]["dqkv_dense"], runs[0]["dqkv_io"])
    assert same_bits(runs[0]["out"], out_f[live.reshape(-1).to(dev)])


# ------------------------------------------------------------------------------------------------ f16 attention
def _f16_run(lib, dev, fill, qkv, dout, B, L, H, causal, off=None, dout_packed=None):
    d = 64 * H
    n = lib.clipfs_attention_lse_floats(B, L, H)
    q16, g16 = int(qkv.dtype == torch.float16), int(dout.dtype == torch.float16)
    out = _buf(B * L * d + TAIL, fill, dev)
    out16 = _buf(B * L * d + TAIL, fill, dev, torch.float16)
    lse, work = _buf(n + TAIL, fill, dev), _buf(n + TAIL, fill, dev)
    assert lib.clipfs_attention_f16_fwd(qkv.data_ptr(), q16, out.data_ptr(), out16.data_ptr(), lse.data_ptr(), B, L, H,
                                        int(causal), _st()) == 0
    rows = B * L if off is None else dout_packed.shape[0]
    dqkv = _buf(rows * 3 * d + TAIL, fill, dev)
    dqkv16 = _buf(rows * 3 * d + TAIL, fill, dev, torch.float16)
    if off is None:
        assert lib.clipfs_attention_f16_bwd(qkv.data_ptr(), q16, dout.data_ptr(), g16, out.data_ptr(), lse.data_ptr(),
                                            dqkv.data_ptr(), dqkv16.data_ptr(), work.data_ptr(), B, L, H, int(causal), _st()) == 0
    else:
        g16 = int(dout_packed.dtype == torch.float16)
        assert lib.clipfs_attention_f16_bwd_packed(qkv.data_ptr(), q16, dout_packed.data_ptr(), g16, out.data_ptr(),
                                                   lse.data_ptr(), dqkv.data_ptr(), dqkv16.data_ptr(), work.data_ptr(),
                                                   off.data_ptr(), B, L, H, _st()) == 0
    torch.cuda.synchronize()
    for name, t, m in (("out", out, B * L * d), ("out16", out16, B * L * d), ("lse", lse, n), ("work", work, n),
                       ("dqkv", dqkv, rows * 3 * d), ("dqkv16", dqkv16, rows * 3 * d)):
        assert _keeps(t[m:], fill), f"{name}: tail written"
    return {"out": out[:B * L * d].clone(), "out16": out16[:B * L * d].clone(), "lse": lse[:n].clone(),
            "dqkv": dqkv[:rows * 3 * d].clone(), "dqkv16": dqkv16[:rows * 3 * d].clone()}


@pytest.mark.parametrize("L,family,qkv_f16,dout_f16", [(77, "f16_short", 0, 0), (77, "f16_short", 0, 1), (77, "f16_short", 1, 0),
                                                        (77, "f16_short", 1, 1), (289, "f16_long", 1, 1)])
def test_attention_f16(dev, L, family, qkv_f16, dout_f16):
    from clipfs import _lib
    lib = _lib.load()
    B, H = 2, 2
    for direction in ("fwd", "bwd"):
        assert _lib.attention_f16_plan(direction, B, L, H, True)["family"] == family
    qkv = _randn(B * L, 3 * 64 * H, seed=300 + L).to(dev)
    dout = _randn(B * L, 64 * H, seed=400 + L).to(dev)
    qkv = qkv.half() if qkv_f16 else qkv
    dout = dout.half() if dout_f16 else dout
    assert_same_runs([_f16_run(lib, dev, f, qkv, dout, B, L, H, True) for f in FILLS])


@pytest.mark.parametrize("dout_f16", [0, 1])
def test_attention_f16_packed(dev, dout_f16):
    """clipfs_attention_f16_bwd_packed over the dense forward's records; dout and dqkv packed with guard rows."""
    from clipfs import _lib
    lib = _lib.load()
    B, L, H = len(PACK_LENS), 77, 2
    d = 64 * H
    assert lib.clipfs_attention_f16_bwd_packed_ok(L, 1)
    assert _lib.attention_f16_plan("bwd_packed", B, L, H, True)["family"] == "f16_short"
    off, R, _ = _pack_off(dev)
    qkv = _randn(B * L, 3 * d, seed=21).to(dev).half()
    dout = _randn(R, d, seed=22)
    runs = []
    for fill in FILLS:
        dp_all, dp = _guarded(dout, fill, dev, torch.float16 if dout_f16 else torch.float32)
        runs.append(_f16_run(lib, dev, fill, qkv, dp, B, L, H, True, off=off, dout_packed=dp))
    assert_same_runs(runs)


# ------------------------------------------------------------------------------------------------------------ LoRA
# (rows, width, segw, r, nseg, family, extras)
LORA = [
    (150, 192, 192, 2, 3, "row", {}),
    (45, 512, 512, 4, 3, "mfma", dict(p=0.25, keep=True, mask=5)),
    (45, 512, 512, 17, 3, "mfma", {}),
    (333, 512, 512, 48, 3, "mfma", dict(frozen=True)),
    (300, 128, 512, 64, 1, "mfma", {}),
    (45, 512, 128, 4, 1, "mfma", dict(x_act=True)),
    (45, 1024, 1024, 16, 3, "mfma", dict(f16dy=True)),
]


def _lora_bwd_call(lib, dev, fill, inp, rows, width, segw, r, nseg, mask, p, seed, kb, x_act, f16dy, frozen, want_dx, rect):
    """One backward with dt and work poisoned (work: the larger of the size query and the plan's written size, plus a
    tail; everything behind the plan's work_floats must keep its fill) and dA / dB / dx pre-filled with seeded values."""
    from clipfs import _lib
    plan = _lib.lora_plan("bwd_f16dy" if f16dy else "bwd", rows, width, segw, r, nseg, x_act=x_act, keep_bits=kb is not None,
                          frozen=frozen, dx=want_dx)
    bound = lib.clipfs_lora_bwd_work_floats2(rows, width, segw, r, nseg)
    if segw == width:
        assert bound == lib.clipfs_lora_bwd_work_floats(rows, width, r, nseg)
    assert plan["work_floats"] <= bound
    work = _buf(bound + TAIL, fill, dev)
    dt = _buf(rows * nseg * r + TAIL, fill, dev)
    dA = None if frozen else _randn(nseg * r, width, seed=31).to(dev)
    dB = None if frozen else _randn(nseg * segw, r, seed=32).to(dev)
    dx = _randn(rows, width, seed=33).to(dev) if want_dx else None
    ptr = lambda t: None if t is None else t.data_ptr()
    dy = inp["dy16"] if f16dy else inp["dy"]
    common = (dy.data_ptr(), inp["x"].data_ptr(), inp["t"].data_ptr(), inp["A"].data_ptr(), inp["B"].data_ptr(), dt.data_ptr(),
              ptr(dA), ptr(dB), ptr(dx), rows, width, segw, r)
    if rect:
        rc = lib.clipfs_lora_bwd_xact(*common, 0.5, p, seed, 7, 3, int(x_act), work.data_ptr(), _st())
    else:
        fn = lib.clipfs_lora_bwd_f16dy if f16dy else lib.clipfs_lora_bwd
        rc = fn(*common, nseg, mask, 0.5, p, seed, 7, 3, ptr(kb), work.data_ptr(), _st())
    assert rc == 0, lib.clipfs_last_error()
    torch.cuda.synchronize()
    assert _keeps(work[plan["work_floats"]:], fill), "work: written past the plan's work_floats"
    assert _keeps(dt[rows * nseg * r:], fill), "dt: tail written"
    dt = dt[:rows * nseg * r].view(rows, nseg * r).clone()
    for s in range(nseg):
        if not (mask >> s) & 1:
            assert not bool(dt[:, s * r:(s + 1) * r].any()), "dt: a segment outside seg_mask must be exact zero"
    res = {"dt": dt}
    for name, t in (("dA", dA), ("dB", dB), ("dx", dx)):
        if t is not None:
            res[name] = t
    return res


@pytest.mark.parametrize("rows,width,segw,r,nseg,family,extra", LORA)
def test_lora(dev, rows, width, segw, r, nseg, family, extra):
    from clipfs import _lib, ops
    lib = _lib.load()
    p, mask = extra.get("p", 0.0), extra.get("mask", (1 << nseg) - 1)
    x_act, f16dy, rect = extra.get("x_act", False), extra.get("f16dy", False), segw != width
    seed = 0x1234ABCD5 if p > 0 else 0
    assert _lib.lora_plan("down", rows, width, segw, r, nseg)["family"] == family
    assert _lib.lora_plan("bwd", rows, width, segw, r, nseg, x_act=x_act)["family"] == family
    if extra.get("keep"):
        assert lib.clipfs_lora_keep_bits_ok(width, segw, r, nseg) == 1
    if f16dy:
        assert lib.clipfs_lora_bwd_f16dy_ok(width, segw, r, nseg) == 1
    x = _randn(rows, width, seed=1).to(dev)
    A = _randn(nseg * r, width, seed=2, scale=width ** -0.5).to(dev)
    Bm = _randn(nseg * segw, r, seed=3, scale=0.1).to(dev)
    dy = _randn(rows, nseg * segw, seed=4).to(dev)
    # the down-projection: t is a fresh allocation inside the wrapper; keep bits are integers (never poisoned)
    downs, kbs = [], []
    for fill in FILLS:
        kb = ops.lora_keep_bits(rows, width, dev) if extra.get("keep") else None
        with poisoned(fill):
            t = ops.lora_down(x, A, r, nseg, seg_mask=mask, p=p, seed=seed, stream_base=7, row0=3, keep_bits=kb)
        for s in range(nseg):
            if not (mask >> s) & 1:
                assert not bool(t[:, s * r:(s + 1) * r].any()), "t: a segment outside seg_mask must be exact zero"
        downs.append({"t": t} if kb is None else {"t": t, "keep": kb})
        kbs.append(kb)
    assert_same_runs(downs)
    inp = dict(x=x, A=A, B=Bm, dy=dy, dy16=dy.half(), t=downs[0]["t"])
    variants = [(False, True)]
    if extra.get("frozen"):
        variants += [(True, True), (True, False)]  # frozen, and frozen with no dx
    res = {}
    for frozen, want_dx in variants:
        runs = [_lora_bwd_call(lib, dev, f, inp, rows, width, segw, r, nseg, mask, p, seed, kbs[0], x_act, f16dy, frozen,
                               want_dx, rect) for f in FILLS]
        assert_same_runs(runs)
        res[(frozen, want_dx)] = runs[0]
    if extra.get("frozen"):  # dt / dx of a frozen adapter are documented bitwise those of the call with slots
        assert same_bits(res[(True, True)]["dt"], res[(False, True)]["dt"])
        assert same_bits(res[(True, True)]["dx"], res[(False, True)]["dx"])
        assert same_bits(res[(True, False)]["dt"], res[(False, True)]["dt"])


# ------------------------------------------------------------------------------------ smaller kernels with work buffers
@pytest.mark.parametrize("rows,cols,segw", [(1000, 771, 0), (12800, 2304, 768)])
def test_bias_grad(dev, rows, cols, segw):
    from clipfs import _lib
    lib = _lib.load()
    need = lib.clipfs_bias_grad_work_floats(rows, cols)
    assert need > 0
    x = _randn(rows, cols, seed=rows).to(dev)
    runs = []
    for fill in FILLS:
        n_out = 3 if segw else 1
        outs = [_randn(segw or cols, seed=50 + s).to(dev) for s in range(n_out)] + [None] * (3 - n_out)
        if segw:
            outs[1] = None  # a frozen segment is skipped
        work = _buf(need + TAIL, fill, dev)
        ptr = lambda t: None if t is None else t.data_ptr()
        assert lib.clipfs_bias_grad(x.data_ptr(), cols, rows, cols, segw, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]),
                                    work.data_ptr(), _st()) == 0
        torch.cuda.synchronize()
        assert _keeps(work[need:], fill), "work: tail written"
        runs.append({f"out{s}": o for s, o in enumerate(outs) if o is not None})
    assert_same_runs(runs)


@pytest.mark.parametrize("width", [128, 1024])
def test_layernorm(dev, width):
    from clipfs import ops
    rows = 131
    x = _randn(rows, width, seed=width).to(dev)
    gamma = (1.0 + 0.1 * _randn(width, seed=1)).to(dev)
    beta = _randn(width, seed=2, scale=0.1).to(dev)
    dy = _randn(rows, width, seed=3).to(dev)
    dres = _randn(rows, width, seed=4).to(dev)
    runs = []
    for fill in FILLS:
        with poisoned(fill):
            y, mean, rstd = ops.layernorm_fwd(x, gamma, beta, save_stats=True)
            dx = ops.layernorm_bwd(dy, x, gamma, mean, rstd, dres=dres)
            dx0 = ops.layernorm_bwd(dy, x, gamma, mean, rstd)
        runs.append(dict(y=y, mean=mean, rstd=rstd, dx=dx, dx0=dx0))
    assert_same_runs(runs)


def test_mta(dev):
    from clipfs import ops
    V, d, Cn, n_img = 65, 64, 12, 2
    g = torch.Generator().manual_seed(4)
    base = torch.randn(n_img, 1, d, generator=g, dtype=torch.float64)
    feats = torch.nn.functional.normalize(base + 0.35 * torch.randn(n_img, V, d, generator=g, dtype=torch.float64), dim=-1)
    text = torch.nn.functional.normalize(torch.randn(Cn, d, generator=g, dtype=torch.float64), dim=-1)
    feats, text = feats.float().to(dev), text.float().to(dev)
    runs = []
    for fill in FILLS:
        with poisoned(fill):
            mode, logits = ops.mta(feats, text)
        runs.append(dict(mode=mode, logits=logits))
    assert_same_runs(runs)


def test_tpt_objective(dev):
    from clipfs import ops
    from tpt_ref import tpt_inputs
    n_img, V, d, Cn, K = 8, 6, 64, 2, 2
    pairs = [tpt_inputs(V, Cn, d, seed=70 + i) for i in range(n_img)]
    feats = torch.stack([f for f, _ in pairs]).float().to(dev).contiguous()
    text = torch.stack([t for _, t in pairs]).float().to(dev).contiguous()
    runs = []
    for fill in FILLS:
        with poisoned(fill):
            loss, sel, dtext, ent = ops.tpt_objective(feats, text, K, want_entropy=True)
            loss2, _, dtext2, _ = ops.tpt_objective(feats, text, K, selected=sel)  # a later step of the episode
        runs.append(dict(loss=loss, selected=sel, dtext=dtext, entropy=ent, loss2=loss2, dtext2=dtext2))
    assert_same_runs(runs)
    assert same_bits(runs[0]["loss"], runs[0]["loss2"]) and same_bits(runs[0]["dtext"], runs[0]["dtext2"])


def test_grad_sumsq_clip_decide(dev):
    """n = 4099: more than one workgroup's partial and a scalar tail.  The work buffer is float64, which the poisoning
    allocator leaves alone, so it is filled here."""
    from clipfs import _lib, ops
    n = 4099
    need = _lib.load().clipfs_grad_sumsq_work_doubles(n)
    g = _randn(n, seed=9).to(dev)
    runs = []
    for fill in FILLS:
        work = torch.full((need + 8,), fill, device=dev, dtype=torch.float64)
        ops.grad_sumsq(g, work)
        st = ops.new_clip_state(dev)
        ops.clip_decide(work, n, 1.0, st)
        torch.cuda.synchronize()
        assert _keeps(work[need:], fill), "work: tail written"
        runs.append(dict(partials=work[:need].clone(), record=st))
    assert_same_runs(runs)


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
def test_cross_entropy(dev, scaled):
    """clipfs_cross_entropy and clipfs_cross_entropy_scaled: loss_rows (scratch), loss_sum, dlogits and the hit count
    are fresh allocations of the wrapper."""
    from clipfs import ops
    rows, classes = 37, 403
    logits = _randn(rows, classes, seed=5, scale=3.0).to(dev)
    target = torch.randint(0, classes, (rows,), generator=torch.Generator().manual_seed(6)).to(dev)
    runs = []
    for fill in FILLS:
        state = ops.new_scaler_state(1024.0, dev) if scaled else None
        with poisoned(fill):
            loss, dl, correct = ops.cross_entropy(logits, target, grad_scale=1.0 / rows, scale_state=state)
        runs.append(dict(loss=loss, dlogits=dl, correct=correct))
    assert_same_runs(runs)
