"""What the GEMM matrix tests share (test_gemm_matrix_gpu.py: fp32 / bf16x3 / f16 plane kernels, test_gemm_f16_matrix_gpu.py:
the f16 x f16 kernels): the NaN sentinels, matrices embedded in sentinel-filled wider ones, and the ONE fp64 restatement
of the epilogue of include/clipfs.h."""
import torch

SENT = 0x7FC5A5A5          # a quiet fp32 NaN nobody computes
SENT16 = 0x7E5A            # the same for f16 (exponent all ones, quiet bit set)


# ------------------------------------------------------------------ the one reference
def quick_gelu(x):
    return x * torch.sigmoid(1.702 * x)


def quick_gelu_grad(x):
    s = torch.sigmoid(1.702 * x)
    return s + 1.702 * x * s * (1.0 - s)


def ref_gemm(a, b, *, alpha=1.0, bias=None, lora=None, act=0, aux_in=None, residual=None, acc=None, lora_f16=False):
    """fp64 restatement of the epilogue order of include/clipfs.h.  a [M,K], b [N,K]; lora = (t [M, nseg r], lb [N, r],
    segment width, scale); returns (C, pre_activation) (the latter None unless act == 1).  `acc` = a @ b.T when the
    caller already has it.  `lora_f16` rounds the adapter operands the way the f16 x f16 kernel does."""
    assert all(x is None or (x.dtype == torch.float64 and not x.is_cuda) for x in (a, b, bias, aux_in, residual, acc))
    v = (a @ b.t() if acc is None else acc) * alpha
    if bias is not None:
        v = v + bias
    if lora is not None:
        t, lb, seg, scale = lora
        if lora_f16:  # the f16 x f16 kernel: t and lora_scale * lora_b (an fp32 product) go through f16 into the MFMAs
            t = t.float().half().double()
            lb = (lb.float() * torch.tensor(scale, dtype=torch.float32)).half().double()
            scale = 1.0
        r = lb.shape[1]
        N = v.shape[1]
        v = v.clone()
        for s in range(t.shape[1] // r):
            lo, hi = s * seg, min((s + 1) * seg, N)
            if lo < hi:
                v[:, lo:hi] += scale * (t[:, s * r:(s + 1) * r] @ lb[lo:hi].t())
    pre = None
    if act == 1:
        pre = v
        v = quick_gelu(v)
    elif act == 2:
        v = v * quick_gelu_grad(aux_in)
    if residual is not None:
        v = v + residual
    if act == 3:
        v = torch.clamp(v, min=0.0)
    return v, pre


def _nan_f32(*shape, dev):
    return torch.full(shape, SENT, dtype=torch.int32, device=dev).view(torch.float32)


def _embed(x, rows, ld, dev, row_index=None):
    """x [m, n] inside a NaN matrix [rows, ld] (at `row_index` rows, default the first m)"""
    buf = _nan_f32(rows, ld, dev=dev)
    if row_index is None:
        buf[:x.shape[0], :x.shape[1]] = x.to(dev)
    else:
        buf[:, :x.shape[1]][row_index.to(dev)] = x.to(dev)
    return buf


def _untouched(buf):
    return bool((buf.view(torch.int32) == SENT).all().item())


def _err(got, want):
    """max |got - want|; NaN (an element never written, or computed from padding) counts as infinite"""
    d = (got.double() - want).abs()
    return float("inf") if torch.isnan(d).any() else d.max().item()


def _nan_f16(*shape, dev):
    return torch.full(shape, SENT16, dtype=torch.int16, device=dev).view(torch.float16)


def _embed16(x, rows, ld, dev):
    """f16 x [m, n] inside an f16 NaN matrix [rows, ld]"""
    buf = _nan_f16(rows, ld, dev=dev)
    buf[:x.shape[0], :x.shape[1]] = x.to(dev)
    return buf


def _bits(buf):
    return buf.view(torch.int16 if buf.dtype == torch.float16 else torch.int32)


def _sent_of(buf):
    return SENT16 if buf.dtype == torch.float16 else SENT
