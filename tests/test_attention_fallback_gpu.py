"""The exact-fp32 attention kernels that are the whole fallback of the dispatch plan (csrc/attention.hip) and that no
default call of the other suites reaches, against the fp64 reference of test_kernels_gpu.py::test_attention (the
oracle's sdpa and causal mask), with its budgets: 2e-5 on the forward and the log-sum-exp, 5e-5 on the backward relative
to max(1, max |grad|).

  * streaming kernels at 1025 tokens: the shortest length that reaches them by default, with a one-row last group of four;
  * the same kernels for an `out` / `dqkv` that is not 16-byte aligned (direct calls, NaN sentinels around the result);
  * the softmax-recomputing backward (no out / lse), one shape per LMAX instance plus the 64 / 65 block-size edge.

Measured on an MI355X (worst max abs error over the shapes of each test, this library | the one before the plan):
  streaming 1025       forward 3.2e-07, lse 8.3e-07, backward 4.5e-06 of a 1.6e-04 budget | the same kernels, the same figures
  misaligned 50 / 130  forward 5.1e-07, lse 6.7e-07, backward 1.4e-06 | forward 4.5e-07, backward 6.2e-07 at 130 on the
                       retired LDS kernels; at 50 its register forward left lse unwritten, so there is nothing to compare
  recomputing          backward 1.0e-06 of a 2.3e-04 budget | the same kernel, the same figures
so every budget is the one of test_attention, none widened."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

FWD_TOL, BWD_TOL = 2e-5, 5e-5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _reference(B, L, H, causal):
    """(qkv, out, lse, dout, dqkv) in fp64, computed once per shape and never modified"""
    from oracle import clip_oracle as O
    d = H * 64
    g = torch.Generator().manual_seed(1000 * L + 10 * H + B)
    qkv = torch.randn(B * L, 3 * d, generator=g, dtype=torch.float64).requires_grad_()
    do = torch.randn(B * L, d, generator=g, dtype=torch.float64)
    q, k, v = [qkv[:, i * d:(i + 1) * d].reshape(B, L, H, 64).permute(0, 2, 1, 3) for i in range(3)]
    mask = O.build_causal_mask(L, torch.float64) if causal else None
    o = O.sdpa(q, k, v, mask).permute(0, 2, 1, 3).reshape(B * L, d)
    lse = torch.logsumexp((q @ k.transpose(-1, -2)) * 0.125 + (mask if causal else 0), -1).reshape(-1)
    o.backward(do)
    return qkv.detach(), o.detach(), lse.detach(), do, qkv.grad


def _check(what, got, want, tol):
    err = (got.detach().double().cpu() - want).abs().max().item()
    print(f"{what}: max abs err {err:.3e} (budget {tol:.3e})")
    assert err <= tol, f"{what}: max abs err {err:.3e} > {tol:.3e}"


def _bwd_tol(grad):
    return BWD_TOL * max(1.0, grad.abs().max().item())


@pytest.mark.parametrize("B,L,H,causal", [(1, 1025, 2, False), (1, 1025, 1, True)])
def test_streaming_kernels(dev, B, L, H, causal):
    from clipfs import ops
    qkv, o, lse_ref, do, grad = _reference(B, L, H, causal)
    qd = qkv.float().to(dev)
    out, lse = ops.attention_fwd(qd, B, L, H, causal, want_lse=True)
    _check("streaming forward", out, o, FWD_TOL)
    _check("streaming lse", lse, lse_ref, FWD_TOL)
    assert torch.equal(ops.attention_fwd(qd, B, L, H, causal), out), "the forward without lse is the same kernel"
    dq = ops.attention_bwd(qd, do.float().to(dev), B, L, H, causal, out=out, lse=lse)
    _check("streaming backward", dq, grad, _bwd_tol(grad))


@pytest.mark.parametrize("B,L,H,causal", [(2, 50, 2, True), (1, 130, 1, False)])
def test_misaligned_out_and_dqkv(dev, B, L, H, causal):
    """out and dqkv one float into a larger buffer: the result is right and nothing around it is written."""
    from clipfs import _lib
    lib = _lib.load()
    qkv, o, lse_ref, do, grad = _reference(B, L, H, causal)
    qd, dod = qkv.float().to(dev), do.float().to(dev)
    nan = float("nan")
    obuf = torch.full((o.numel() + 9,), nan, device=dev)
    gbuf = torch.full((qkv.numel() + 9,), nan, device=dev)
    lse = torch.empty(B * H * L, device=dev)
    work = torch.empty_like(lse)
    assert qd.data_ptr() % 16 == 0 and dod.data_ptr() % 16 == 0 and obuf.data_ptr() % 16 == 0 and gbuf.data_ptr() % 16 == 0
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.clipfs_attention_fwd(qd.data_ptr(), obuf.data_ptr() + 4, lse.data_ptr(), B, L, H, int(causal), st))
    _lib.check(lib.clipfs_attention_bwd(qd.data_ptr(), dod.data_ptr(), obuf.data_ptr() + 4, lse.data_ptr(), gbuf.data_ptr() + 4,
                                        work.data_ptr(), B, L, H, int(causal), st))
    torch.cuda.synchronize()
    for buf, n in ((obuf, o.numel()), (gbuf, qkv.numel())):
        assert torch.isnan(buf[0]).item() and torch.isnan(buf[1 + n:]).all().item(), "a sentinel was overwritten"
    _check("misaligned forward", obuf[1:1 + o.numel()].reshape(o.shape), o, FWD_TOL)
    _check("misaligned lse", lse, lse_ref, FWD_TOL)
    _check("misaligned backward", gbuf[1:1 + qkv.numel()].reshape(qkv.shape), grad, _bwd_tol(grad))


@pytest.mark.parametrize("B,L,H,causal", [(3, 31, 1, True), (1, 65, 2, False), (2, 81, 1, True), (2, 96, 2, True)])
def test_recomputing_backward(dev, B, L, H, causal):
    """no out / lse from the forward: LMAX 64 (256 threads), 80, 96 and 96 (512 threads)"""
    from clipfs import ops
    qkv, _, _, do, grad = _reference(B, L, H, causal)
    dq = ops.attention_bwd(qkv.float().to(dev), do.float().to(dev), B, L, H, causal)
    _check("recomputing backward", dq, grad, _bwd_tol(grad))


def test_these_calls_get_the_fallback_kernels():
    """host-only: the plan of each call above"""
    from clipfs import _lib
    for causal in (False, True):
        assert _lib.attention_plan("fwd", 1, 1025, 2, causal)["family"] == "stream"
        assert _lib.attention_plan("bwd", 1, 1025, 2, causal)["family"] == "stream"
    for L in (50, 130):
        assert _lib.attention_plan("fwd", 2, L, 2, True, aligned=False)["family"] == "stream"
        assert _lib.attention_plan("bwd", 2, L, 2, True, aligned=False)["family"] == "stream"
    assert [_lib.attention_plan("bwd", 2, L, 2, True, stats=False)["lmax"] for L in (31, 65, 81, 96)] == [64, 80, 96, 96]
