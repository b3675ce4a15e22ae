"""fp16-mode MFMA attention past 288 tokens (up to ops.attention_f16_max_seq()): the long-sequence kernels cut the own side
into runs of tiles, one workgroup each, and stream the other side through LDS in chunks.  The error model is that of the
short kernels (P and dS rounded to f16 as MFMA operands, statistics and accumulators fp32), so the tolerances are the ones
tests/test_kernels_gpu.py states for them: output 2e-3 absolute, lse 1e-3, gradients 1e-2 of the largest entry -- an
emulation of that rounding model on the CPU stays below 3.7e-4 / 1e-6 / 3.6e-4 on the shapes below.

Shapes (batch, seq, heads, causal): one token past the old bound; a whole number of tiles; ViT-L/14 at 336 px (577 tokens,
two heads, two images); the bound itself; two causal cases (the CLIP text tower never gets this long, but the entry points
take the flag)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

MAX_SEQ = "max_seq"  # resolved through ops.attention_f16_max_seq() inside the test: no library call at collection time
SHAPES = [(1, 289, 1, False), (1, 320, 1, False), (2, 577, 2, False), (1, MAX_SEQ, 1, False), (1, 300, 2, True),
          (1, 577, 1, True)]


def _seq(seq):
    from clipfs import ops
    return ops.attention_f16_max_seq() if seq == MAX_SEQ else seq


def _attn_ref64(qkv, batch, seq, heads, causal=False):
    d = heads * 64
    x = qkv.double().view(batch, seq, 3, heads, 64)
    q, k, v = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2)
    s = q @ k.transpose(-1, -2) * 0.125
    if causal:
        s = s + torch.full((seq, seq), float("-inf"), dtype=torch.float64, device=s.device).triu(1)
    lse = torch.logsumexp(s, -1)
    o = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(batch * seq, d)
    return o, lse.reshape(-1)


def test_max_seq_is_past_vit_l14_336():
    from clipfs import ops
    assert ops.attention_f16_max_seq() >= 577


@pytest.mark.parametrize("batch,seq,heads,causal", SHAPES)
def test_attention_f16_long_fwd(batch, seq, heads, causal):
    """Forward vs an fp64 reference on the SAME f16-rounded q, k, v: 2e-3 absolute on the output, 1e-3 on the log-sum-exp;
    qkv passed as an f16 tensor gives the same bits."""
    from clipfs import _lib, ops
    seq = _seq(seq)
    assert _lib.attention_f16_plan("fwd", batch, seq, heads, causal)["family"] == "f16_long"
    g = torch.Generator().manual_seed(seq)
    qkv = torch.randn(batch * seq, 3 * heads * 64, generator=g).half().float().cuda()
    out, lse = ops.attention_f16_fwd(qkv, batch, seq, heads, causal)
    ro, rl = _attn_ref64(qkv, batch, seq, heads, causal)
    e_out, e_lse = (out.double() - ro).abs().max().item(), (lse.double() - rl).abs().max().item()
    print(f"fwd {batch}x{seq}x{heads} causal={causal}: |out - ref| = {e_out:.3e}, |lse - ref| = {e_lse:.3e}")
    assert e_out < 2e-3
    assert e_lse < 1e-3
    out_h, lse_h = ops.attention_f16_fwd(qkv.half(), batch, seq, heads, causal)
    assert torch.equal(out_h, out) and torch.equal(lse_h, lse)


def _bwd16(qkv, dout, out, lse, batch, seq, heads, causal, want32):
    """The C entry point with the f16 result requested: returns (dqkv or None, dqkv16)."""
    from clipfs import _lib
    dqkv = torch.empty(qkv.shape, device=qkv.device, dtype=torch.float32) if want32 else None
    dqkv16 = torch.empty(qkv.shape, device=qkv.device, dtype=torch.float16)
    work = torch.empty_like(lse)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    _lib.check(_lib.load().clipfs_attention_f16_bwd(p(qkv), int(qkv.dtype == torch.float16), p(dout),
                                                    int(dout.dtype == torch.float16), p(out), p(lse), p(dqkv), p(dqkv16),
                                                    p(work), batch, seq, heads, int(causal),
                                                    torch.cuda.current_stream().cuda_stream), "attention_f16_bwd")
    return dqkv, dqkv16


@pytest.mark.parametrize("batch,seq,heads,causal", SHAPES)
def test_attention_f16_long_bwd(batch, seq, heads, causal):
    """Backward vs fp64 autograd on the same f16-rounded inputs: 1e-2 of the largest gradient entry.  The four storage
    combinations (qkv fp32 / f16 x dO fp32 / f16) give the same bits, and the f16-only result (no fp32 dqkv) is the
    rounded fp32 result."""
    from clipfs import _lib, ops
    seq = _seq(seq)
    assert _lib.attention_f16_plan("bwd", batch, seq, heads, causal)["family"] == "f16_long"
    g = torch.Generator().manual_seed(seq + 7)
    qkv = torch.randn(batch * seq, 3 * heads * 64, generator=g).half().float().cuda()
    dout = torch.randn(batch * seq, heads * 64, generator=g).half().float().cuda()
    out, lse = ops.attention_f16_fwd(qkv, batch, seq, heads, causal)
    dqkv = ops.attention_f16_bwd(qkv, dout, out, lse, batch, seq, heads, causal)
    assert torch.equal(ops.attention_f16_bwd(qkv.half(), dout, out, lse, batch, seq, heads, causal), dqkv)
    assert torch.equal(ops.attention_f16_bwd(qkv, dout.half(), out, lse, batch, seq, heads, causal), dqkv)
    assert torch.equal(ops.attention_f16_bwd(qkv.half(), dout.half(), out, lse, batch, seq, heads, causal), dqkv)
    both32, both16 = _bwd16(qkv.half(), dout.half(), out, lse, batch, seq, heads, causal, want32=True)
    none32, only16 = _bwd16(qkv.half(), dout.half(), out, lse, batch, seq, heads, causal, want32=False)
    assert none32 is None and torch.equal(both32, dqkv)
    assert torch.equal(both16, dqkv.half()) and torch.equal(only16, dqkv.half())
    x = qkv.double().requires_grad_(True)
    ro, _ = _attn_ref64(x, batch, seq, heads, causal)
    (ro * dout.double()).sum().backward()
    ref = x.grad
    e, scale = (dqkv.double() - ref).abs().max().item(), ref.abs().max().item()
    print(f"bwd {batch}x{seq}x{heads} causal={causal}: |dqkv - ref| = {e:.3e} = {e / scale:.3e} of the largest entry")
    assert e < 1e-2 * scale


def test_reproducible_and_heads_independent():
    """Two calls give equal bits, and head (b, h) of a (3, 577, 2) call equals the same head computed alone as a (1, 577, 1)
    call bit for bit: a wrong run, chunk or grid index mixes heads or tokens."""
    from clipfs import _lib, ops
    batch, seq, heads = 3, 577, 2
    for d, b, h in (("fwd", batch, heads), ("bwd", batch, heads), ("fwd", 1, 1), ("bwd", 1, 1)):
        assert _lib.attention_f16_plan(d, b, seq, h, False)["family"] == "f16_long"
    g = torch.Generator().manual_seed(seq + 13)
    qkv = torch.randn(batch * seq, 3 * heads * 64, generator=g).half().float().cuda()
    dout = torch.randn(batch * seq, heads * 64, generator=g).half().float().cuda()
    out, lse = ops.attention_f16_fwd(qkv, batch, seq, heads)
    dqkv = ops.attention_f16_bwd(qkv, dout, out, lse, batch, seq, heads)
    out2, lse2 = ops.attention_f16_fwd(qkv, batch, seq, heads)
    assert torch.equal(out2, out) and torch.equal(lse2, lse)
    assert torch.equal(ops.attention_f16_bwd(qkv, dout, out, lse, batch, seq, heads), dqkv)
    q5, g5 = qkv.view(batch, seq, 3, heads, 64), dout.view(batch, seq, heads, 64)
    for b in range(batch):
        for h in range(heads):
            one = q5[b, :, :, h].reshape(seq, 192).contiguous()
            gone = g5[b, :, h].contiguous()
            o1, l1 = ops.attention_f16_fwd(one, 1, seq, 1)
            assert torch.equal(o1, out.view(batch, seq, heads, 64)[b, :, h])
            assert torch.equal(l1, lse.view(batch, heads, seq)[b, h])
            d1 = ops.attention_f16_bwd(one, gone, o1, l1, 1, seq, 1)
            assert torch.equal(d1.view(seq, 3, 64), dqkv.view(batch, seq, 3, heads, 64)[b, :, :, h])


def test_seq_past_the_bound_is_refused():
    """A host-side check: nothing is launched, the message names the sequence length and the bound."""
    from clipfs import _lib, ops
    bound = ops.attention_f16_max_seq()
    seq = bound + 1
    qkv = torch.zeros(seq, 192).cuda()
    with pytest.raises(_lib.ClipfsError) as e:
        ops.attention_f16_fwd(qkv, 1, seq, 1)
    assert f"seq {seq}" in str(e.value) and str(bound) in str(e.value)
    with pytest.raises(_lib.ClipfsError) as e:
        ops.attention_f16_bwd(qkv, torch.zeros(seq, 64).cuda(), torch.zeros(seq, 64).cuda(), torch.zeros(seq).cuda(), 1, seq, 1)
    assert f"seq {seq}" in str(e.value) and str(bound) in str(e.value)
