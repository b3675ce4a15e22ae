"""Exact-fp32 MFMA attention past 288 tokens (up to ops.attention_mfma_max_seq()): the long-sequence kernels cut the own
side into runs of 32-token tiles, one workgroup each, and pass the other side's transposed image through LDS in chunks.

1. Neither cut changes the arithmetic: a wave walks the same tiles in the same order with the same tile body as in the
   short kernels, so for seq <= 288 the hooked long kernels (explicit chunk size and run length) must give the BITS of
   ops.attention_fwd / attention_bwd, whatever the cut.
2. Past the old bound the default dispatch is compared with an fp64 reference on unit-normal inputs, at the tolerances
   tests/test_kernels_gpu.py::test_attention states for exact-fp32 attention: out and lse 2e-5, dqkv 5e-5 absolute.  A
   plain fp32 evaluation on the CPU stays below 6e-7 / 5.8e-7 / 2.9e-6 on these shapes (17x margin or more); a dropped
   tile or chunk misses by orders of magnitude.
3. Two runs give equal bits.
4. One token past the bound the streaming kernels still answer, within the same tolerances."""
import pytest
import torch

pytestmark = pytest.mark.gpu

MAX_SEQ = "max_seq"  # resolved through ops.attention_mfma_max_seq() inside the test: no library call at collection time
TOL_OUT, TOL_LSE, TOL_DQKV = 2e-5, 2e-5, 5e-5


def _seq(seq):
    from clipfs import ops
    return ops.attention_mfma_max_seq() if seq == MAX_SEQ else seq


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


def _inputs(batch, seq, heads, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(batch * seq, 3 * heads * 64, generator=g).cuda()
    dout = torch.randn(batch * seq, heads * 64, generator=g).cuda()
    return qkv, dout


def _errors(qkv, dout, out, lse, dqkv, batch, seq, heads, causal):
    x = qkv.double().requires_grad_(True)
    ro, rl = _attn_ref64(x, batch, seq, heads, causal)
    (ro * dout.double()).sum().backward()
    return ((out.double() - ro.detach()).abs().max().item(), (lse.double() - rl.detach()).abs().max().item(),
            (dqkv.double() - x.grad).abs().max().item())


# ---------------------------------------------------------------- 1. chunking and runs are arithmetic-neutral
NEUTRAL_SHAPES = [(1, 130, 1, True), (2, 257, 2, False), (1, 288, 3, False), (1, 288, 1, True)]
_short = {}


def _short_result(batch, seq, heads, causal):
    """The short MFMA kernels' result, computed once per shape and left unchanged."""
    key = (batch, seq, heads, causal)
    if key not in _short:
        from clipfs import ops
        qkv, dout = _inputs(batch, seq, heads, seed=seq + 3)
        out, lse = ops.attention_fwd(qkv, batch, seq, heads, causal, want_lse=True)
        dqkv = ops.attention_bwd(qkv, dout, batch, seq, heads, causal, out=out, lse=lse)
        _short[key] = (qkv, dout, out, lse, dqkv)
    return _short[key]


@pytest.mark.parametrize("chunk,run", [(64, 1), (96, 2), (160, 3), (288, "RUN")])
@pytest.mark.parametrize("batch,seq,heads,causal", NEUTRAL_SHAPES)
def test_chunks_and_runs_do_not_change_a_bit(batch, seq, heads, causal, chunk, run):
    """130 tokens in chunks of 64: a partial last tile in a partial last chunk; 257 tokens in runs of 2: a short last run; the
    causal shapes: waves with nothing visible in a chunk, on both sides of the diagonal."""
    from clipfs import ops
    run = ops.ATTENTION_MFMA_LONG_RUN if run == "RUN" else run
    qkv, dout, out, lse, dqkv = _short_result(batch, seq, heads, causal)
    lout, llse = ops.attention_mfma_long_fwd(qkv, batch, seq, heads, causal, chunk_tokens=chunk, run_tiles=run)
    assert torch.equal(lout, out)
    assert torch.equal(llse, lse)
    ldqkv = ops.attention_mfma_long_bwd(qkv, dout, out, lse, batch, seq, heads, causal, chunk_tokens=chunk, run_tiles=run)
    assert torch.equal(ldqkv, dqkv)


# ---------------------------------------------------------------- 2. parity past the old bound, default dispatch
LONG_SHAPES = [(1, 289, 1, False), (1, 320, 1, False), (2, 353, 3, False), (2, 577, 2, False), (1, MAX_SEQ, 1, False),
               (1, 300, 2, True), (1, 577, 1, True)]


@pytest.mark.parametrize("batch,seq,heads,causal", LONG_SHAPES)
def test_parity_past_288_tokens(batch, seq, heads, causal):
    from clipfs import ops
    seq = _seq(seq)
    qkv, dout = _inputs(batch, seq, heads, seed=seq)
    out, lse = ops.attention_fwd(qkv, batch, seq, heads, causal, want_lse=True)
    dqkv = ops.attention_bwd(qkv, dout, batch, seq, heads, causal, out=out, lse=lse)
    e_out, e_lse, e_dqkv = _errors(qkv, dout, out, lse, dqkv, batch, seq, heads, causal)
    print(f"{batch}x{seq}x{heads} causal={causal}: |out - ref| = {e_out:.3e}, |lse - ref| = {e_lse:.3e}, "
          f"|dqkv - ref| = {e_dqkv:.3e}")
    assert e_out < TOL_OUT
    assert e_lse < TOL_LSE
    assert e_dqkv < TOL_DQKV
    # the default dispatch IS the long kernels with the default cut
    lout, llse = ops.attention_mfma_long_fwd(qkv, batch, seq, heads, causal)
    assert torch.equal(lout, out) and torch.equal(llse, lse)
    if seq == 577 and not causal:  # inference: no lse buffer
        assert torch.equal(ops.attention_fwd(qkv, batch, seq, heads, causal), out)


# ---------------------------------------------------------------- 3. run-to-run determinism
@pytest.mark.parametrize("batch,seq,heads,causal", [(2, 577, 2, False), (1, 577, 1, True)])
def test_two_runs_give_equal_bits(batch, seq, heads, causal):
    from clipfs import ops
    qkv, dout = _inputs(batch, seq, heads, seed=seq + 13)
    out, lse = ops.attention_fwd(qkv, batch, seq, heads, causal, want_lse=True)
    dqkv = ops.attention_bwd(qkv, dout, batch, seq, heads, causal, out=out, lse=lse)
    out2, lse2 = ops.attention_fwd(qkv, batch, seq, heads, causal, want_lse=True)
    assert torch.equal(out2, out) and torch.equal(lse2, lse)
    assert torch.equal(ops.attention_bwd(qkv, dout, batch, seq, heads, causal, out=out, lse=lse), dqkv)


# ---------------------------------------------------------------- 4. the bound
def test_one_token_past_the_bound_runs_the_streaming_kernels():
    from clipfs import _lib, ops
    batch, seq, heads, causal = 1, ops.attention_mfma_max_seq() + 1, 1, False
    qkv, dout = _inputs(batch, seq, heads, seed=seq)
    out, lse = ops.attention_fwd(qkv, batch, seq, heads, causal, want_lse=True)
    dqkv = ops.attention_bwd(qkv, dout, batch, seq, heads, causal, out=out, lse=lse)
    e_out, e_lse, e_dqkv = _errors(qkv, dout, out, lse, dqkv, batch, seq, heads, causal)
    print(f"{batch}x{seq}x{heads}: |out - ref| = {e_out:.3e}, |lse - ref| = {e_lse:.3e}, |dqkv - ref| = {e_dqkv:.3e}")
    assert e_out < TOL_OUT
    assert e_lse < TOL_LSE
    assert e_dqkv < TOL_DQKV
    with pytest.raises(_lib.ClipfsError):  # and the MFMA hook refuses that length
        ops.attention_mfma_long_fwd(qkv, batch, seq, heads, causal)
