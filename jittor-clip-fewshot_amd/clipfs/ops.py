"""Tensor-level wrappers over the C ABI (include/clipfs.h).  PyTorch is used only to own device
memory and streams; every function here enqueues hand-written HIP kernels on the current stream.
All tensors must be contiguous fp32 CUDA(ROCm) tensors unless stated otherwise."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._lib import GemmArgs, check


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    assert t.is_cuda, "clipfs ops need device tensors (there is no CPU path)"
    return t.data_ptr()


def _f32(t: torch.Tensor) -> torch.Tensor:
    assert t.dtype == torch.float32 and t.is_contiguous(), (t.dtype, t.is_contiguous())
    return t


_COUNTERS = {}


def _gemm_counters(device, n: int) -> torch.Tensor:
    """Zeroed split-K arrival counters for a stand-alone GEMM call: cached per (device, stream) -- launches on one
    stream are ordered and every launch leaves the counters zero."""
    key = (device.index, _stream())
    buf = _COUNTERS.get(key)
    if buf is None or buf.numel() < n:
        buf = torch.zeros(max(n, 4096), device=device, dtype=torch.int32)
        _COUNTERS[key] = buf
    return buf


def gemm_nt(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None, *, bias=None, residual=None,
            act: int = 0, aux_out=None, aux_in=None, alpha: float = 1.0, lora_t=None, lora_b=None,
            lora_seg_width: int = 0, lora_scale: float = 0.0, split_k: bool = True, b_planes=None,
            a16: Optional[torch.Tensor] = None, out16: Optional[torch.Tensor] = None, only16: bool = False,
            aux_f16: bool = False) -> torch.Tensor:
    """out = epi(alpha * a @ b.T); a [M,K], b [N,K].  ``a16`` (f16 [M,K]) with f16 ``b_planes`` selects the
    f16 x f16 kernel (``a`` may then be None); ``out16`` (f16 [M,N]) receives an f16 copy of the result.  That kernel
    refuses ``alpha != 1`` together with ``lora_t`` (its adapter product would be scaled by alpha)."""
    if a is not None:
        _f32(a)
    _f32(b)
    M, K = (a16 if a is None else a).shape
    N = b.shape[0]
    assert b.shape[1] == K
    if out is None and not only16:
        out = torch.empty(M, N, device=b.device, dtype=torch.float32)
    g = _lib.new_gemm_args()
    g.A, g.B, g.C = _p(a), _p(b), (None if only16 else _p(out))
    if a16 is not None:
        assert a16.dtype == torch.float16 and a16.is_contiguous() and tuple(a16.shape) == (M, K)
        g.A_f16 = _p(a16)
    if out16 is not None:
        assert out16.dtype == torch.float16 and out16.is_contiguous() and tuple(out16.shape) == (M, N)
        g.C_f16 = _p(out16)
    g.M, g.N, g.K = M, N, K
    g.lda, g.ldb, g.ldc = K, K, N
    g.alpha = alpha
    g.bias = _p(bias)
    g.residual = _p(residual)
    g.ldres = N
    g.act = act
    g.aux_out = _p(aux_out)
    g.aux_in = _p(aux_in)
    g.aux_f16 = int(aux_f16)  # f16 x f16 kernel: aux_out / aux_in are f16 tensors (fp16 storage of the pre-activation)
    if lora_t is not None:
        r = lora_b.shape[1]
        g.lora_t, g.lora_b = _p(_f32(lora_t)), _p(_f32(lora_b))
        g.lora_r = r
        g.lora_nseg = lora_t.shape[1] // r
        g.lora_seg_width = lora_seg_width or N
        g.lora_scale = lora_scale
    g.B_planes = _p(b_planes)
    if b_planes is not None:
        g.b_format = 2 if b_planes.dtype == torch.float16 else 1
    lib = _lib.load()
    ws = None
    nws = lib.clipfs_gemm_workspace_floats(M, N, K) if split_k else 0
    if nws:
        ws = torch.empty(nws, device=b.device, dtype=torch.float32)
        g.workspace, g.workspace_floats = _p(ws), nws
        ncnt = lib.clipfs_gemm_counter_ints(M, N, K)
        if ncnt and a is not None and b_planes is None:
            cnt = _gemm_counters(b.device, ncnt)
            g.counters, g.counters_ints = _p(cnt), cnt.numel()
    check(lib.clipfs_gemm_nt(C.byref(g), _stream()), "gemm_nt")
    return out16 if only16 else out


def split_bf16(w: torch.Tensor) -> torch.Tensor:
    """hi/lo bf16 planes of a frozen fp32 weight: int16 tensor [2, *w.shape] (bit patterns)."""
    _f32(w)
    planes = torch.empty((2,) + tuple(w.shape), device=w.device, dtype=torch.int16)
    check(_lib.load().clipfs_split_bf16(_p(w), _p(planes), w.numel(), _stream()), "split_bf16")
    return planes


def to_f16(w: torch.Tensor) -> torch.Tensor:
    """f16 plane of a frozen fp32 weight (fp16 MFMA mode)."""
    _f32(w)
    out = torch.empty(w.shape, device=w.device, dtype=torch.float16)
    check(_lib.load().clipfs_convert_f16(_p(w), _p(out), w.numel(), _stream()), "convert_f16")
    return out


PLANE_FORMATS = {"fp32": 0, "bf16x3": 1, "fp16": 2}  # clipfs_tower.weight_format / clipfs_lora_merge plane_format


def empty_planes(w: torch.Tensor, fmt: int) -> Optional[torch.Tensor]:
    """An unwritten 16-bit image of ``w`` in plane format ``fmt``, shaped as ``split_bf16`` / ``to_f16`` return it."""
    if fmt == 1:
        return torch.empty((2,) + tuple(w.shape), device=w.device, dtype=torch.int16)
    if fmt == 2:
        return torch.empty(w.shape, device=w.device, dtype=torch.float16)
    return None


def lora_merge(jobs, r: int, scale: float, fmt: int = 0) -> None:
    """ONE clipfs_lora_merge launch over ``jobs`` = [(w [n,k], a [nseg*r,k], b [n,r], nseg, seg_mask, out [n,k], planes |
    None)]: out = w + scale * b a per segment (segments outside ``seg_mask``: the bits of w), ``planes`` = the 16-bit
    image of out in plane format ``fmt`` (``empty_planes``).  w is read only.  The host table is validated by the library;
    its device copy is uploaded here."""
    table = (_lib.MergeJob * len(jobs))()
    tile0 = 0
    dev = None
    for rec, (w, a, b, nseg, seg_mask, out, planes) in zip(table, jobs):
        _f32(w), _f32(a), _f32(b), _f32(out)
        n, k = w.shape
        assert tuple(out.shape) == (n, k) and tuple(a.shape) == (nseg * r, k) and tuple(b.shape) == (n, r), \
            (tuple(w.shape), tuple(a.shape), tuple(b.shape), tuple(out.shape), nseg, r)
        if planes is not None:
            assert planes.is_contiguous() and planes.numel() * planes.element_size() == (4 if fmt == 1 else 2) * n * k
        rec.w, rec.a, rec.b, rec.out, rec.planes = _p(w), _p(a), _p(b), _p(out), _p(planes)
        rec.n, rec.k, rec.nseg, rec.seg_mask, rec.tile0 = n, k, nseg, seg_mask, tile0
        tile0 += _lib.merge_job_tiles(n, k, nseg)
        dev = w.device
    if not jobs:
        raise ValueError("lora_merge: empty job table")
    table_dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
    check(_lib.load().clipfs_lora_merge(table, _p(table_dev), len(jobs), C.sizeof(_lib.MergeJob), r, float(scale), fmt,
                                        _stream()), "lora_merge")
    # table_dev was allocated on this stream: its storage is handed out again only to work ordered behind the launch


def patch_embed(images: torch.Tensor, conv_w: torch.Tensor, pos: torch.Tensor, x: torch.Tensor, tokens: int) -> None:
    """x[b, 1+p, :] = conv(images)[b, :, p] + pos[1+p]  (im2col-free GEMM on the NCHW batch)."""
    _f32(images), _f32(conv_w), _f32(pos), _f32(x)
    B, ch, R, _ = images.shape
    width, _, ps, _ = conv_w.shape
    assert ch == 3
    P = (R // ps) ** 2
    g = _lib.new_gemm_args()
    g.A, g.B, g.C = _p(images), _p(conv_w), _p(x)
    g.M, g.N, g.K = B * P, width, 3 * ps * ps
    g.lda, g.ldb, g.ldc = 0, 3 * ps * ps, width
    g.alpha = 1.0
    g.residual = _p(pos)
    g.ldres = width
    g.a_mode = 1
    g.img_res, g.patch, g.out_tokens = R, ps, tokens
    check(_lib.load().clipfs_gemm_nt(C.byref(g), _stream()), "patch_embed")


def layernorm_fwd(x, gamma, beta, *, ldx=None, rows=None, save_stats=False, eps=1e-5):
    width = gamma.numel()
    if rows is None:
        rows = x.numel() // width
    ldx = ldx or width
    y = torch.empty(rows, width, device=x.device, dtype=torch.float32)
    mean = rstd = None
    if save_stats:
        mean = torch.empty(rows, device=x.device, dtype=torch.float32)
        rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
    check(_lib.load().clipfs_layernorm_fwd(_p(x), ldx, _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), rows, width,
                                           eps, _stream()), "layernorm_fwd")
    return (y, mean, rstd) if save_stats else y


def layernorm_fwd_lora(x, gamma, beta, A, r, nseg=3, *, seg_mask=None, p=0.0, seed=0, stream_base=0, row0=0, eps=1e-5,
                       keep_bits=None):
    """LayerNorm + adapter down-projection in one pass: returns (y, t, mean, rstd)."""
    width = gamma.numel()
    rows = x.numel() // width
    lib = _lib.load()
    if not lib.clipfs_layernorm_fwd_lora_ok(width, r, nseg):
        raise ValueError(f"layernorm_fwd_lora: width {width} r {r} nseg {nseg} is not covered")
    y = torch.empty(rows, width, device=x.device, dtype=torch.float32)
    t = torch.empty(rows, nseg * r, device=x.device, dtype=torch.float32)
    mean = torch.empty(rows, device=x.device, dtype=torch.float32)
    rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
    if seg_mask is None:
        seg_mask = (1 << nseg) - 1
    check(lib.clipfs_layernorm_fwd_lora(_p(_f32(x)), width, _p(gamma), _p(beta), _p(y), None, _p(mean), _p(rstd), rows, width,
                                        eps, _p(_f32(A)), _p(t), r, nseg, seg_mask, p, seed, stream_base, row0, _p(keep_bits),
                                        _stream()),
          "layernorm_fwd_lora")
    return y, t, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, *, ldx=None, dres=None, dx=None, lddx=None):
    width = gamma.numel()
    rows = dy.numel() // width
    ldx = ldx or width
    lddx = lddx or width
    if dx is None:
        dx = torch.empty(rows, width, device=dy.device, dtype=torch.float32)
    check(_lib.load().clipfs_layernorm_bwd(_p(dy), _p(x), ldx, _p(gamma), _p(mean), _p(rstd), _p(dres), _p(dx), lddx,
                                           rows, width, _stream()), "layernorm_bwd")
    return dx


def attention_fwd(qkv, batch, seq, heads, causal, want_lse=False):
    out = torch.empty(batch * seq, heads * 64, device=qkv.device, dtype=torch.float32)
    lib = _lib.load()
    n = lib.clipfs_attention_lse_floats(batch, seq, heads) if want_lse else 0
    lse = torch.empty(n, device=qkv.device, dtype=torch.float32) if n else None
    check(lib.clipfs_attention_fwd(_p(_f32(qkv)), _p(out), _p(lse), batch, seq, heads, int(causal), _stream()),
          "attention_fwd")
    return (out, lse) if want_lse else out


def attention_mfma_max_seq() -> int:
    """Longest sequence the exact-fp32 MFMA attention takes; attention_fwd / attention_bwd run streaming VALU kernels past it."""
    return _lib.load().clipfs_attention_mfma_max_seq()


ATTENTION_MFMA_LONG_RUN = 4  # most 32-token tiles per run (= waves per workgroup) of the long-sequence fp32 MFMA kernels


def attention_mfma_long_fwd(qkv, batch, seq, heads, causal=False, chunk_tokens=0, run_tiles=0, want_lse=True):
    """The long-sequence fp32 MFMA forward (96 < seq <= attention_mfma_max_seq()) with an explicit cut: the other side in
    chunks of at most chunk_tokens tokens (a multiple of 32 up to 288), the own side in runs of at most run_tiles tiles
    (1 .. ATTENTION_MFMA_LONG_RUN); 0 = the default attention_fwd uses past 288 tokens.  The cut changes no bit of the
    result.  Returns (out, lse), or out alone with want_lse=False."""
    out = torch.empty(batch * seq, heads * 64, device=qkv.device, dtype=torch.float32)
    lse = torch.empty(batch * heads * seq, device=qkv.device, dtype=torch.float32) if want_lse else None
    check(_lib.load().clipfs_attention_mfma_long_fwd(_p(_f32(qkv)), _p(out), _p(lse), batch, seq, heads, int(causal),
                                                     chunk_tokens, run_tiles, _stream()), "attention_mfma_long_fwd")
    return (out, lse) if want_lse else out


def attention_mfma_long_bwd(qkv, dout, out, lse, batch, seq, heads, causal=False, chunk_tokens=0, run_tiles=0):
    """dqkv of attention_mfma_long_fwd (same bounds, same meaning of chunk_tokens and run_tiles)."""
    dqkv = torch.empty_like(qkv)
    work = torch.empty_like(lse)
    check(_lib.load().clipfs_attention_mfma_long_bwd(_p(_f32(qkv)), _p(_f32(dout)), _p(out), _p(lse), _p(dqkv), _p(work),
                                                     batch, seq, heads, int(causal), chunk_tokens, run_tiles, _stream()),
          "attention_mfma_long_bwd")
    return dqkv


def attention_f16_max_seq() -> int:
    """Longest sequence the fp16-mode MFMA attention takes (a longer one is refused before anything is launched)."""
    return _lib.load().clipfs_attention_f16_max_seq()


def attention_f16_fwd(qkv, batch, seq, heads, causal=False):
    """fp16-mode MFMA attention (seq <= attention_f16_max_seq(); K / V streamed through LDS past 288 tokens): returns
    (out, lse)."""
    out = torch.empty(batch * seq, heads * 64, device=qkv.device, dtype=torch.float32)
    lse = torch.empty(batch * heads * seq, device=qkv.device, dtype=torch.float32)
    f16 = qkv.dtype == torch.float16
    check(_lib.load().clipfs_attention_f16_fwd(_p(qkv if f16 else _f32(qkv)), int(f16), _p(out), None, _p(lse), batch, seq,
                                               heads, int(causal), _stream()), "attention_f16_fwd")
    return out, lse


def attention_f16_bwd(qkv, dout, out, lse, batch, seq, heads, causal=False):
    """dqkv of attention_f16_fwd (same bound on seq); qkv and dout may each be fp32 or f16."""
    f16 = qkv.dtype == torch.float16
    dqkv = torch.empty(qkv.shape, device=qkv.device, dtype=torch.float32)
    work = torch.empty_like(lse)
    g16 = dout.dtype == torch.float16  # dO as its f16 image (what the fp16-storage tower hands over) or fp32
    assert dout.is_contiguous()
    check(_lib.load().clipfs_attention_f16_bwd(_p(qkv if f16 else _f32(qkv)), int(f16), _p(dout if g16 else _f32(dout)), int(g16),
                                               _p(out), _p(lse), _p(dqkv), None, _p(work), batch, seq, heads, int(causal), _stream()),
          "attention_f16_bwd")
    return dqkv


def attention_bwd(qkv, dout, batch, seq, heads, causal, out=None, lse=None):
    dqkv = torch.empty_like(qkv)
    work = torch.empty_like(lse) if lse is not None else None
    check(_lib.load().clipfs_attention_bwd(_p(_f32(qkv)), _p(_f32(dout)), _p(out), _p(lse), _p(dqkv), _p(work), batch,
                                           seq, heads, int(causal), _stream()), "attention_bwd")
    return dqkv


def lora_keep_bits(rows, width, device):
    """Buffer for the dropout masks an adapted projection records in its forward (uint16 per float4 of the input)."""
    return torch.zeros(rows, width // 4, device=device, dtype=torch.int16)


def lora_down(x, A, r, nseg, seg_mask=None, p=0.0, seed=0, stream_base=0, row0=0, keep_bits=None):
    rows, width = x.shape
    t = torch.empty(rows, nseg * r, device=x.device, dtype=torch.float32)
    if seg_mask is None:
        seg_mask = (1 << nseg) - 1
    check(_lib.load().clipfs_lora_down(_p(_f32(x)), _p(_f32(A)), _p(t), rows, width, r, nseg, seg_mask, p, seed,
                                       stream_base, row0, _p(keep_bits), _stream()), "lora_down")
    return t


def lora_bwd(dy, x, t, A, B, dA, dB, *, dx=None, scale, p=0.0, seed=0, stream_base=0, seg_mask=None, row0=0, keep_bits=None):
    rows, width = x.shape
    nseg = dy.shape[1] // width
    r = B.shape[1]
    if seg_mask is None:
        seg_mask = (1 << nseg) - 1
    lib = _lib.load()
    nwork = lib.clipfs_lora_bwd_work_floats(rows, width, r, nseg)
    work = torch.empty(nwork, device=x.device, dtype=torch.float32)
    dt = torch.empty(rows, nseg * r, device=x.device, dtype=torch.float32)
    if dy.dtype == torch.float16:  # fp16 storage mode: the f16 image of the incoming gradient (matrix-core shapes only)
        assert dy.is_contiguous()
        check(lib.clipfs_lora_bwd_f16dy(_p(dy), _p(_f32(x)), _p(_f32(t)), _p(_f32(A)), _p(_f32(B)), _p(dt), _p(dA),
                                        _p(dB), _p(dx), rows, width, width, r, nseg, seg_mask, scale, p, seed, stream_base,
                                        row0, _p(keep_bits), _p(work), _stream()), "lora_bwd_f16dy")
        return dt
    check(lib.clipfs_lora_bwd(_p(_f32(dy)), _p(_f32(x)), _p(_f32(t)), _p(_f32(A)), _p(_f32(B)), _p(dt), _p(dA),
                              _p(dB), _p(dx), rows, width, width, r, nseg, seg_mask, scale, p, seed, stream_base,
                              row0, _p(keep_bits), _p(work), _stream()), "lora_bwd")
    return dt


def lora_bwd_rect(dy, x, t, A, B, dA, dB, *, dx=None, scale, p=0.0, seed=0, stream_base=0, row0=0, x_act=False):
    """Backward of ONE adapter whose output width (``dy`` [rows, out]) may differ from its input width (``x`` [rows, in]):
    the MLP linears' adapters (clipfs_lora_bwd_xact).  ``x_act``: ``x`` holds the pre-activation u and the adapter read
    QuickGELU(u) -- applied as x is loaded, and ``dx`` then receives the gradient wrt QuickGELU(u).  dA / dB None = frozen.
    Returns dt [rows, r]."""
    rows, width = x.shape
    segw = dy.shape[1]
    r = B.shape[1]
    lib = _lib.load()
    work = torch.empty(lib.clipfs_lora_bwd_work_floats2(rows, width, segw, r, 1), device=x.device, dtype=torch.float32)
    dt = torch.empty(rows, r, device=x.device, dtype=torch.float32)
    check(lib.clipfs_lora_bwd_xact(_p(_f32(dy)), _p(_f32(x)), _p(_f32(t)), _p(_f32(A)), _p(_f32(B)), _p(dt), _p(dA), _p(dB),
                                   _p(dx), rows, width, segw, r, scale, p, seed, stream_base, row0, int(bool(x_act)), _p(work),
                                   _stream()), "lora_bwd_xact")
    return dt


def gelu_bwd_inplace(dg, u):
    """dg *= QuickGELU'(u), in place (clipfs_gelu_bwd_inplace)."""
    assert dg.is_contiguous() and u.is_contiguous() and dg.numel() == u.numel()
    check(_lib.load().clipfs_gelu_bwd_inplace(_p(_f32(dg)), _p(_f32(u)), dg.numel(), _stream()), "gelu_bwd_inplace")
    return dg


def vit_fill_special(x, class_emb, pos, vpt, batch, tokens, n_patch):
    n_vpt = 0 if vpt is None else vpt.shape[0]
    check(_lib.load().clipfs_vit_fill_special(_p(x), _p(class_emb), _p(pos), _p(vpt), batch, tokens, n_patch, n_vpt,
                                              class_emb.numel(), _stream()), "vit_fill_special")


def text_embed(ids, table, pos, ctx=None):
    n, seq = ids.shape
    width = table.shape[1]
    assert ids.dtype == torch.int64 and ids.is_contiguous()
    x = torch.empty(n * seq, width, device=table.device, dtype=torch.float32)
    n_ctx = 0 if ctx is None else ctx.shape[0]
    check(_lib.load().clipfs_text_embed(_p(ids), _p(table), _p(pos), _p(ctx), n_ctx, _p(x), n, seq, width, _stream()),
          "text_embed")
    return x


def token_rows_grad(dx, dtok, n, seq, first):
    n_tok, width = dtok.shape
    check(_lib.load().clipfs_token_rows_grad(_p(dx), _p(dtok), n, seq, width, n_tok, first, _stream()),
          "token_rows_grad")


def matmul_small(a, b, M, N, K, sam, sak, sbk, sbn, alpha=1.0, out=None):
    if out is None:
        out = torch.empty(M, N, device=a.device, dtype=torch.float32)
    check(_lib.load().clipfs_matmul_small(_p(a), _p(b), _p(out), M, N, K, sam, sak, sbk, sbn, alpha, _stream()),
          "matmul_small")
    return out


def add_rows_(dst: torch.Tensor, src: torch.Tensor, zero_idx: torch.Tensor) -> torch.Tensor:
    """dst += src for two contiguous [n, width] tensors (clipfs_add_seq_rows with one row per sequence); ``zero_idx``: at
    least n int32 zeros on the device (``Engine._class_rows``)."""
    n, width = src.shape
    assert dst.shape == src.shape and dst.is_contiguous() and zero_idx.dtype == torch.int32 and zero_idx.numel() >= n
    check(_lib.load().clipfs_add_seq_rows(_p(_f32(src)), _p(zero_idx), _p(_f32(dst)), n, 1, width, _stream()), "add_seq_rows")
    return dst


def eot_index(ids: torch.Tensor) -> torch.Tensor:
    """idx[c] = position of the EOT token (largest id, first maximum) of caption c, int32 [n] (jclip/model.py:213-214)."""
    assert ids.is_cuda and ids.dtype == torch.int64 and ids.is_contiguous()
    n, seq = ids.shape
    idx = torch.empty(n, device=ids.device, dtype=torch.int32)
    check(_lib.load().clipfs_eot_index(_p(ids), _p(idx), n, seq, _stream()), "eot_index")
    return idx


def gather_eot(x, ids):
    n, seq = ids.shape
    width = x.shape[-1]
    out = torch.empty(n, width, device=x.device, dtype=torch.float32)
    idx = torch.empty(n, device=x.device, dtype=torch.int32)
    check(_lib.load().clipfs_gather_eot(_p(x), _p(ids), _p(out), _p(idx), n, seq, width, _stream()), "gather_eot")
    return out, idx


def scatter_rows(dy, idx, seq, out=None):
    n, width = dy.shape
    dx = out if out is not None else torch.empty(n * seq, width, device=dy.device, dtype=torch.float32)
    check(_lib.load().clipfs_scatter_rows(_p(_f32(dy)), _p(idx), _p(dx), n, seq, width, _stream()), "scatter_rows")
    return dx


def l2norm_fwd(x, save_inv=False, out=None):
    rows, width = x.shape
    y = torch.empty_like(x) if out is None else out
    assert y.is_contiguous() and y.shape == x.shape and y.dtype == torch.float32
    inv = torch.empty(rows, device=x.device, dtype=torch.float32) if save_inv else None
    check(_lib.load().clipfs_l2norm_fwd(_p(_f32(x)), _p(y), _p(inv), rows, width, _stream()), "l2norm_fwd")
    return (y, inv) if save_inv else y


def l2norm_bwd(dy, y, inv):
    rows, width = y.shape
    dx = torch.empty_like(y)
    check(_lib.load().clipfs_l2norm_bwd(_p(_f32(dy)), _p(y), _p(inv), _p(dx), rows, width, _stream()), "l2norm_bwd")
    return dx


def class_mean_fwd(emb, classes, templates, out=None):
    width = emb.shape[1]
    if out is None:
        out = torch.empty(classes, width, device=emb.device, dtype=torch.float32)
    assert out.is_contiguous() and tuple(out.shape) == (classes, width)
    check(_lib.load().clipfs_class_mean_fwd(_p(_f32(emb)), _p(out), classes, templates, width, _stream()),
          "class_mean_fwd")
    return out


def class_mean_bwd(emb, dout, classes, templates):
    demb = torch.empty_like(emb)
    check(_lib.load().clipfs_class_mean_bwd(_p(_f32(emb)), _p(_f32(dout)), _p(demb), classes, templates, emb.shape[1],
                                            _stream()), "class_mean_bwd")
    return demb


def cross_entropy(logits, target, want_grad=True, grad_scale=1.0, scale_state=None):
    """returns (loss_sum [1], dlogits or None, correct [1] int32).  ``scale_state`` (a loss-scaling record,
    ``new_scaler_state``): dlogits additionally carries the record's current scale; the loss and the hit count do not."""
    rows, classes = logits.shape
    assert target.dtype == torch.int64
    dl = torch.empty_like(logits) if want_grad else None
    loss_rows = torch.empty(2 * rows, device=logits.device, dtype=torch.float32)
    loss_sum = torch.empty(1, device=logits.device, dtype=torch.float32)
    correct = torch.empty(1, device=logits.device, dtype=torch.int32)
    if scale_state is None:
        check(_lib.load().clipfs_cross_entropy(_p(_f32(logits)), _p(target), _p(dl), _p(loss_rows), _p(loss_sum),
                                               _p(correct), rows, classes, grad_scale, _stream()), "cross_entropy")
    else:
        check(_lib.load().clipfs_cross_entropy_scaled(_p(_f32(logits)), _p(target), _p(dl), _p(loss_rows), _p(loss_sum),
                                                      _p(correct), rows, classes, grad_scale, _p(_scaler(scale_state)),
                                                      _stream()), "cross_entropy_scaled")
    return loss_sum, dl, correct


def topk(logits, k):
    rows, classes = logits.shape
    labels = torch.empty(rows, k, device=logits.device, dtype=torch.int32)
    check(_lib.load().clipfs_topk(_p(_f32(logits)), _p(labels), rows, classes, k, _stream()), "topk")
    return labels


def channel_affine(x, scale1, bias1):
    y = torch.empty_like(x)
    check(_lib.load().clipfs_channel_affine(_p(_f32(x)), _p(scale1), _p(bias1), _p(y), x.shape[0], x.shape[1],
                                            _stream()), "channel_affine")
    return y


def logit_normalize(z):
    out = torch.empty_like(z)
    work = torch.empty(2, device=z.device, dtype=torch.float32)
    check(_lib.load().clipfs_logit_normalize(_p(_f32(z)), _p(out), _p(work), z.shape[0], z.shape[1], _stream()),
          "logit_normalize")
    return out


def logit_normalize_bwd(z, dzn):
    dz = torch.empty_like(z)
    check(_lib.load().clipfs_logit_normalize_bwd(_p(_f32(z)), _p(_f32(dzn)), _p(dz), z.shape[0], z.shape[1], _stream()),
          "logit_normalize_bwd")
    return dz


def colsum(x, y=None, out=None):
    """out[k] = sum_r x[r, k] (* y[r, k]); ``out``: a contiguous fp32 tensor of x.shape[1] elements to write instead."""
    if out is None:
        out = torch.empty(x.shape[1], device=x.device, dtype=torch.float32)
    assert out.is_contiguous() and out.numel() == x.shape[1] and out.dtype == torch.float32
    check(_lib.load().clipfs_colsum(_p(_f32(x)), _p(y), _p(out), x.shape[0], x.shape[1], _stream()), "colsum")
    return out


def bias_grad(x, out, seg_width: int = 0, rows: Optional[int] = None, work: Optional[torch.Tensor] = None):
    """Accumulate column sums of ``x`` [rows, cols] (row stride ``x.stride(0)``, unit column stride) into bias gradient
    slots: ``out`` is one tensor, or a sequence of up to three (None = frozen segment, skipped) receiving the columns
    ``[s * seg_width, (s + 1) * seg_width)``.  ``rows`` (default ``x.shape[0]``) sums a leading part only.  Bitwise
    deterministic (clipfs_bias_grad)."""
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    outs = list(out) if isinstance(out, (list, tuple)) else [out]
    assert 1 <= len(outs) <= 3
    for o in outs:
        assert o is None or (o.dtype == torch.float32 and o.is_contiguous() and o.device == x.device)
    outs += [None] * (3 - len(outs))
    n = x.shape[0] if rows is None else rows
    cols = x.shape[1]
    lib = _lib.load()
    need = lib.clipfs_bias_grad_work_floats(n, cols)
    if need and (work is None or work.numel() < need):
        work = torch.empty(need, device=x.device, dtype=torch.float32)
    check(lib.clipfs_bias_grad(_p(x), x.stride(0), n, cols, seg_width, _p(outs[0]), _p(outs[1]), _p(outs[2]),
                               _p(work) if need else None, _stream()), "bias_grad")


def adamw(p, g, m, v, step, lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_scale=1.0):
    check(_lib.load().clipfs_adamw(_p(p), _p(g), _p(m), _p(v), p.numel(), step, lr, betas[0], betas[1], eps,
                                   weight_decay, grad_scale, _stream()), "adamw")


def new_scaler_state(scale: float, device) -> torch.Tensor:
    """A loss-scaling record (include/clipfs.h, CLIPFS_SCALER_*): fp32 [16] on ``device`` with SCALE = ``scale``,
    INV_SCALE = 1 / scale and everything else zero.  The int32 words are read through ``state.view(torch.int32)``."""
    st = torch.zeros(_lib.SCALER_WORDS, dtype=torch.float32)
    st[_lib.SCALER_SCALE] = scale
    st[_lib.SCALER_INV_SCALE] = 1.0 / scale
    return st.to(device)


def _scaler(state: torch.Tensor) -> torch.Tensor:
    assert state.is_cuda and state.dtype == torch.float32 and state.is_contiguous() and state.numel() >= _lib.SCALER_WORDS
    return state


def grads_nonfinite(g: torch.Tensor, scale_state: torch.Tensor) -> None:
    """Set the record's flag when the flat fp32 buffer ``g`` (any 4-byte aligned slice) holds NaN or +-inf."""
    assert g.dim() == 1
    check(_lib.load().clipfs_grads_nonfinite(_p(_f32(g)), g.numel(), _p(_scaler(scale_state)), _stream()), "grads_nonfinite")


def scaler_decide(scale_state: torch.Tensor, lr=2e-4, betas=(0.9, 0.999), growth_factor=2.0, backoff_factor=0.5,
                  growth_interval=2000) -> None:
    """Turn the flag into the step's decision (apply / skip), the step's AdamW bias corrections and the next scale.
    ``growth_interval=0`` with ``backoff_factor=1.0`` keeps the scale static."""
    check(_lib.load().clipfs_scaler_decide(_p(_scaler(scale_state)), lr, betas[0], betas[1], growth_factor, backoff_factor,
                                           growth_interval, _stream()), "scaler_decide")


def adamw_scaled(p, g, m, v, scale_state, lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
    """``adamw`` with the step number's bias corrections, 1 / scale as the gradient scale and the skip decision taken
    from the record (after ``scaler_decide``)."""
    check(_lib.load().clipfs_adamw_scaled(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, betas[0], betas[1], eps,
                                          weight_decay, _p(_scaler(scale_state)), _stream()), "adamw_scaled")


def new_clip_state(device) -> torch.Tensor:
    """A zeroed clip record (include/clipfs.h, CLIPFS_CLIP_*): fp32 [8] on ``device``."""
    return torch.zeros(_lib.CLIP_WORDS, dtype=torch.float32, device=device)


def _clip(state: torch.Tensor) -> torch.Tensor:
    assert state.is_cuda and state.dtype == torch.float32 and state.is_contiguous() and state.numel() >= _lib.CLIP_WORDS
    return state


def grad_sumsq_work(n: int, device) -> torch.Tensor:
    """The float64 work buffer ``grad_sumsq`` / ``clip_decide`` need for a flat buffer of ``n`` floats."""
    return torch.empty(_lib.load().clipfs_grad_sumsq_work_doubles(n), dtype=torch.float64, device=device)


def grad_sumsq(g: torch.Tensor, work: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Pass 1 of the sum of squares of the flat fp32 buffer ``g`` (any 4-byte aligned slice): one float64 partial per
    workgroup into ``work`` (``grad_sumsq_work``), which is returned.  Bitwise deterministic."""
    assert g.dim() == 1
    need = _lib.load().clipfs_grad_sumsq_work_doubles(g.numel())
    if work is None:
        work = grad_sumsq_work(g.numel(), g.device)
    assert work.is_cuda and work.dtype == torch.float64 and work.is_contiguous() and work.numel() >= need
    check(_lib.load().clipfs_grad_sumsq(_p(_f32(g)), g.numel(), _p(work), _stream()), "grad_sumsq")
    return work


def clip_decide(work: torch.Tensor, n: int, max_norm: float, clip_state: torch.Tensor,
                scale_state: Optional[torch.Tensor] = None) -> None:
    """Add the partials ``grad_sumsq`` left for a buffer of ``n`` floats and write the clip record: NORM (divided by
    the scale of ``scale_state``, after ``scaler_decide``), COEF = min(1, max_norm / (NORM + 1e-6)) and MULT.  A NaN or
    infinite norm gives COEF = 0, as ``torch.nn.utils.clip_grad_norm_(error_if_nonfinite=False)`` does for an infinite
    one; the update is then poisoned by the non-finite entries themselves: ``loss_scale`` is what skips such a step."""
    assert work.is_cuda and work.dtype == torch.float64 and work.is_contiguous()
    assert work.numel() >= _lib.load().clipfs_grad_sumsq_work_doubles(n)
    check(_lib.load().clipfs_clip_decide(_p(work), n, max_norm, None if scale_state is None else _p(_scaler(scale_state)),
                                         _p(_clip(clip_state)), _stream()), "clip_decide")


def adamw_ext(p, g, m, v, step, lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_scale=1.0,
              scale_state=None, clip_state=None, ema_shadow=None, ema_decay=0.999):
    """``adamw`` with three optional device inputs: the loss-scaling record (bias corrections, skip decision and
    1 / scale, as ``adamw_scaled``; ``step`` is then unused), the clip record (its MULT is the gradient multiplier) and
    an EMA shadow [n] updated as ``decay * shadow + (1 - decay) * p_new``.  A skipped step writes nothing at all."""
    if ema_shadow is not None:
        assert ema_shadow.shape == p.shape and ema_shadow.device == p.device
        _f32(ema_shadow)
    check(_lib.load().clipfs_adamw_ext(_p(p), _p(g), _p(m), _p(v), p.numel(), step, lr, betas[0], betas[1], eps,
                                       weight_decay, grad_scale, None if scale_state is None else _p(_scaler(scale_state)),
                                       None if clip_state is None else _p(_clip(clip_state)), _p(ema_shadow), ema_decay,
                                       _stream()), "adamw_ext")


def adamw_tail(p, g, m, v, step, lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_scale=1.0,
               scale_state=None, clip_state=None, ema_shadow=None, ema_decay=0.999, *, tail_n=0, tail_weight_decay=0.0,
               tail_min=float("-inf"), tail_max=float("inf")):
    """``adamw_ext`` whose last ``tail_n`` elements take ``tail_weight_decay`` in place of ``weight_decay`` and are clamped
    to [tail_min, tail_max] after the update (the EMA shadow sees the clamped value): a trained log-temperature at the
    end of the flat buffer, free of decay and held below its cap.  ``tail_n=0`` is bitwise ``adamw_ext``."""
    if ema_shadow is not None:
        assert ema_shadow.shape == p.shape and ema_shadow.device == p.device
        _f32(ema_shadow)
    check(_lib.load().clipfs_adamw_tail(_p(p), _p(g), _p(m), _p(v), p.numel(), step, lr, betas[0], betas[1], eps,
                                        weight_decay, grad_scale, None if scale_state is None else _p(_scaler(scale_state)),
                                        None if clip_state is None else _p(_clip(clip_state)), _p(ema_shadow), ema_decay,
                                        tail_n, tail_weight_decay, tail_min, tail_max, _stream()), "adamw_tail")


def mta(feats, text, want_mode=True, want_logits=True):
    """feats [n_img, V, d] unit rows, text [C, d] unit rows -> (mode [n_img,d], logits [n_img,C])"""
    n_img, V, d = feats.shape
    Cn = text.shape[0]
    lib = _lib.load()
    work = torch.empty(lib.clipfs_mta_work_floats(n_img, V, d, Cn), device=feats.device, dtype=torch.float32)
    mode = torch.empty(n_img, d, device=feats.device, dtype=torch.float32) if want_mode else None
    logits = torch.empty(n_img, Cn, device=feats.device, dtype=torch.float32) if want_logits else None
    check(lib.clipfs_mta(_p(_f32(feats)), _p(_f32(text)), _p(mode), _p(logits), _p(work), n_img, V, d, Cn, _stream()),
          "mta")
    return mode, logits


def l1_loss(a: torch.Tensor, b: torch.Tensor, want_grad: bool = False, grad_scale: float = 1.0):
    """mean |a - b| (slow_pace.py:1654-1655); optionally d/da scaled by grad_scale."""
    a, b = _f32(a).contiguous(), _f32(b).contiguous()
    assert a.shape == b.shape
    loss = torch.empty(1, device=a.device, dtype=torch.float32)
    da = torch.empty_like(a) if want_grad else None
    check(_lib.load().clipfs_l1_loss(_p(a), _p(b), a.numel(), _p(loss), _p(da), grad_scale, _stream()), "l1_loss")
    return (loss, da) if want_grad else loss


def kl_logits(logits: torch.Tensor, target_logits: torch.Tensor, want_grad: bool = False, grad_scale: float = 1.0):
    """per-row KL(softmax(target) || softmax(logits)) (slow_pace.py:1656-1658 with kl_div :1170-1177)."""
    x, t = _f32(logits).contiguous(), _f32(target_logits).contiguous()
    assert x.shape == t.shape and x.dim() == 2
    rows, cols = x.shape
    loss_rows = torch.empty(rows, device=x.device, dtype=torch.float32)
    dx = torch.empty_like(x) if want_grad else None
    check(_lib.load().clipfs_kl_logits(_p(x), _p(t), _p(loss_rows), _p(dx), rows, cols, grad_scale, _stream()), "kl_logits")
    return (loss_rows, dx) if want_grad else loss_rows


def stage2_objective(cos, zs_logits, target, img, zs_img, txt, zs_txt, classes: int, inv_global_batch: float,
                     want_grad: bool = True, scale_state: Optional[torch.Tensor] = None,
                     terms: Optional[torch.Tensor] = None):
    """The stage-2 objective without its head branch (clipfs_stage2_objective): ``cos`` / ``zs_logits`` [B, C],
    ``target`` [B] int64, unit image features ``img`` and their zero-shot counterparts ``zs_img`` [B, d], this rank's unit
    text rows ``txt`` and ``zs_txt`` [C_loc, d] (None or empty: no text row is accounted for here), ``classes`` = C.
    Returns (terms [4] = this rank's share of sim_ce, scl_logits, scl_image, scl_text; correct [1] int32; dcos; dimg;
    dtxt) -- the gradients carry the scale of ``scale_state`` (a loss-scaling record) and are None without
    ``want_grad``; dtxt is None when there is no text row.  ``terms``: a contiguous fp32 tensor whose first four elements
    receive the shares instead of a fresh one."""
    B, C = cos.shape
    d = img.shape[1]
    assert C == classes and zs_logits.shape == cos.shape and zs_img.shape == img.shape == (B, d)
    assert target.dtype == torch.int64 and target.is_contiguous() and target.numel() == B
    n_loc = 0 if txt is None else txt.shape[0]
    if n_loc:
        assert zs_txt is not None and zs_txt.shape == txt.shape == (n_loc, d)
        _f32(txt), _f32(zs_txt)
    else:
        txt = zs_txt = None
    dev = cos.device
    dcos = torch.empty_like(cos) if want_grad else None
    dimg = torch.empty_like(img) if want_grad else None
    dtxt = torch.empty_like(txt) if want_grad and n_loc else None
    work = torch.empty(4 * B + n_loc, device=dev, dtype=torch.float32)
    if terms is None:
        terms = torch.empty(4, device=dev, dtype=torch.float32)
    assert terms.dtype == torch.float32 and terms.is_contiguous() and terms.numel() >= 4 and terms.device == dev
    correct = torch.empty(1, device=dev, dtype=torch.int32)
    check(_lib.load().clipfs_stage2_objective(_p(_f32(cos)), _p(_f32(zs_logits)), _p(target), _p(_f32(img)), _p(_f32(zs_img)),
                                              _p(txt), _p(zs_txt), _p(dcos), _p(dimg), _p(dtxt), _p(work), _p(terms),
                                              _p(correct), B, C, d, n_loc, inv_global_batch,
                                              None if scale_state is None else _p(_scaler(scale_state)), _stream()),
          "stage2_objective")
    return terms, correct, dcos, dimg, dtxt


# ------------------------------------------------------------------------------------------------ cache head
def _cache_shapes(f, keys, offsets):
    B, d = f.shape
    NK = keys.shape[0]
    assert keys.shape[1] == d and offsets.dtype == torch.int32 and offsets.is_contiguous() and offsets.dim() == 1
    return B, NK, offsets.numel() - 1, d


def cache_plan(op: str, B: int, NK: int, C_: int, d: int, nA: int = 1, nB: int = 1):
    """What ``cache_logits`` ("logits"), ``cache_bwd`` ("bwd_dk", "bwd_df") or ``cache_search`` ("search") launch for these
    shapes (host-only): grid, block, lds_bytes, class_chunk, feat_chunk, beta_chunk, alpha_chunk, work_floats."""
    return _lib.cache_plan(op, B, NK, C_, d, nA, nB)


def cache_logits(f, keys, offsets, base=None, alpha=1.0, beta=5.5, out=None):
    """logits [B, C] = base + alpha * (per-class sums of exp(-beta (1 - f keys^T))): the Tip-Adapter cache head in one
    launch.  ``keys`` [NK, d] sorted by class, ``offsets`` int32 [C + 1]; ``base`` and ``out`` may be column slices (row
    stride >= C, unit column stride).  ``out`` must not alias ``base``."""
    B, NK, Cn, d = _cache_shapes(f, keys, offsets)
    if out is None:
        out = torch.empty(B, Cn, device=f.device, dtype=torch.float32)
    for t in (base, out):
        assert t is None or (t.dtype == torch.float32 and tuple(t.shape) == (B, Cn) and t.stride(1) == 1), "base / out"
    check(_lib.load().clipfs_cache_logits(_p(_f32(f)), _p(_f32(keys)), _p(offsets), _p(base), _p(out), B, NK, Cn, d,
                                          0 if base is None else (base.stride(0) if B > 1 else max(base.stride(0), Cn)),
                                          out.stride(0) if B > 1 else max(out.stride(0), Cn), alpha, beta, _stream()),
          "cache_logits")
    return out


def cache_bwd(f, keys, offsets, dlogits, dkeys, alpha=1.0, beta=5.5, want_df=False):
    """Adds the key gradient of ``cache_logits`` for ``dlogits`` [B, C] into ``dkeys`` [NK, d]; returns df [B, d] when
    ``want_df`` (else None)."""
    B, NK, Cn, d = _cache_shapes(f, keys, offsets)
    assert tuple(dlogits.shape) == (B, Cn) and tuple(dkeys.shape) == (NK, d)
    df = torch.empty_like(f) if want_df else None
    check(_lib.load().clipfs_cache_bwd(_p(_f32(f)), _p(_f32(keys)), _p(offsets), _p(_f32(dlogits)), _p(_f32(dkeys)), _p(df),
                                       B, NK, Cn, d, Cn, alpha, beta, _stream()), "cache_bwd")
    return df


def cache_search(f, keys, offsets, base, target, alphas, betas):
    """hits int32 [nB, nA]: per (beta, alpha) cell the rows whose top-1 of ``cache_logits`` equals ``target`` (int64 [B]),
    one launch; ``alphas`` / ``betas`` are fp32 device vectors."""
    B, NK, Cn, d = _cache_shapes(f, keys, offsets)
    assert target.dtype == torch.int64 and target.is_contiguous() and target.numel() == B
    assert base is None or (base.dtype == torch.float32 and tuple(base.shape) == (B, Cn) and base.stride(1) == 1)
    nA, nB = alphas.numel(), betas.numel()
    hits = torch.zeros(nB, nA, device=f.device, dtype=torch.int32)
    check(_lib.load().clipfs_cache_search(_p(_f32(f)), _p(_f32(keys)), _p(offsets), _p(base), _p(target), _p(_f32(alphas)),
                                          _p(_f32(betas)), _p(hits), B, NK, Cn, d,
                                          0 if base is None else (base.stride(0) if B > 1 else max(base.stride(0), Cn)),
                                          nA, nB, _stream()), "cache_search")
    return hits


class CacheLogitsFn(torch.autograd.Function):
    """``cache_logits`` differentiable w.r.t. the keys, the base logits and (when they require grad) the queries."""

    @staticmethod
    def forward(ctx, f, keys, offsets, base, alpha, beta):
        f, keys = f.contiguous(), keys.contiguous()
        ctx.save_for_backward(f, keys, offsets)
        ctx.alpha, ctx.beta = float(alpha), float(beta)
        return cache_logits(f, keys, offsets, base, alpha, beta)

    @staticmethod
    def backward(ctx, dlogits):
        f, keys, offsets = ctx.saved_tensors
        dlogits = dlogits.contiguous()
        dkeys = torch.zeros_like(keys)
        df = cache_bwd(f, keys, offsets, dlogits, dkeys, ctx.alpha, ctx.beta, want_df=ctx.needs_input_grad[0])
        return df, dkeys if ctx.needs_input_grad[1] else None, None, dlogits if ctx.needs_input_grad[3] else None, None, None


# ------------------------------------------------------------------------------------------------ TPT objective
def tpt_objective(feats, text, K, logit_scale=100.0, selected=None, want_grad=True, grad_scale=1.0, want_entropy=False):
    """The test-time prompt tuning objective for ``feats`` [n_img, V, d] (unit view features) and ``text`` [C, d] shared by
    the images or [n_img, C, d] one per image (unit class features): per image the entropy of the softmax averaged over
    the ``K`` views of lowest entropy (ties to the lower view index) and its gradient with respect to ``text``, in at most
    three launches for the whole batch.  ``selected`` (int32 [n_img, K], ascending view index): given, it IS the
    selection (a later step of an episode reuses the first step's); None, it is made and returned.  Returns
    (loss [n_img], selected [n_img, K], dtext [n_img, C, d] = ``grad_scale`` * d loss / d text or None, entropy
    [n_img, V] or None)."""
    assert feats.dim() == 3 and text.dim() in (2, 3), "feats [n_img, V, d], text [C, d] or [n_img, C, d]"
    n_img, V, d = feats.shape
    Cn = text.shape[-2]
    assert text.shape[-1] == d and (text.dim() == 2 or text.shape[0] == n_img), (tuple(feats.shape), tuple(text.shape))
    dev = feats.device
    reuse = selected is not None
    if reuse:
        assert selected.dtype == torch.int32 and selected.is_contiguous() and tuple(selected.shape) == (n_img, K)
    else:
        selected = torch.empty(n_img, max(K, 0), device=dev, dtype=torch.int32)
    lib = _lib.load()
    loss = torch.empty(n_img, device=dev, dtype=torch.float32)
    entropy = torch.empty(n_img, V, device=dev, dtype=torch.float32) if want_entropy else None
    dtext = torch.empty(n_img, Cn, d, device=dev, dtype=torch.float32) if want_grad else None
    work = torch.empty(max(lib.clipfs_tpt_work_floats(n_img, V, d, Cn), 4), device=dev, dtype=torch.float32)
    check(lib.clipfs_tpt_objective(_p(_f32(feats)), _p(_f32(text)), int(text.dim() == 3), _p(selected), int(reuse), K,
                                   logit_scale, grad_scale, _p(loss), _p(entropy), _p(dtext), _p(work), n_img, V, d, Cn,
                                   _stream()), "tpt_objective")
    return loss, selected, dtext, entropy


# ------------------------------------------------------------------------------------------------ TDA
TDA_DEFAULTS = dict(logit_scale=100.0, pos_cap=3, neg_cap=2, pos_alpha=2.0, pos_beta=5.0, neg_alpha=0.117, neg_beta=1.0,
                    ent_lo=0.2, ent_hi=0.5, mask_lo=0.03, mask_hi=1.0)
TDA_MAX_BATCH = 8192  # of clipfs_tda_adapt


def tda_params(C_: int, d: int, **hyper):
    """struct clipfs_tda_params for C classes of d features; ``hyper`` overrides TDA_DEFAULTS (unknown names: KeyError)."""
    unknown = sorted(set(hyper) - set(TDA_DEFAULTS))
    if unknown:
        raise KeyError(f"tda_params: unknown hyper-parameter(s) {', '.join(unknown)}")
    return _lib.new_tda_params(C=C_, d=d, **{**TDA_DEFAULTS, **hyper})


def tda_plan(C_: int, d: int, B: int, update: bool = True, **hyper):
    """What ``tda_adapt`` launches for B samples (host-only): launches (the same for every B and C), launch = {name: (grid_x,
    grid_y, block, lds_bytes)}, lds_bytes, class_chunk, and the element counts of the state and record tensors."""
    return _lib.tda_plan(tda_params(C_, d, **hyper), B, update)


def tda_new_state(C_: int, d: int, pos_cap: int, neg_cap: int, device):
    """An empty TDA state: the fixed-shape device tensors of struct clipfs_tda_state, by name."""
    f32, i64 = torch.float32, torch.int64
    return dict(pos_keys=torch.zeros(C_, pos_cap, d, device=device, dtype=f32),
                pos_ent=torch.full((C_, pos_cap), float("inf"), device=device, dtype=f32),
                pos_seq=torch.full((C_, pos_cap), -1, device=device, dtype=i64),
                neg_keys=torch.zeros(C_, neg_cap, d, device=device, dtype=f32),
                neg_ent=torch.full((C_, neg_cap), float("inf"), device=device, dtype=f32),
                neg_seq=torch.full((C_, neg_cap), -1, device=device, dtype=i64),
                neg_mask=torch.zeros(C_, neg_cap, C_, device=device, dtype=torch.uint8),
                counter=torch.zeros(1, device=device, dtype=i64))


_TDA_STATE_DTYPES = dict(pos_keys=torch.float32, pos_ent=torch.float32, pos_seq=torch.int64, neg_keys=torch.float32,
                         neg_ent=torch.float32, neg_seq=torch.int64, neg_mask=torch.uint8, counter=torch.int64)


def tda_new_record(C_: int, B: int, pos_cap: int, neg_cap: int, device):
    """The per-sample record of one ``tda_adapt`` call (struct clipfs_tda_record): every element is written by the call."""
    i32 = torch.int32
    e = lambda n, dt: torch.empty(n, device=device, dtype=dt)
    return dict(pred=e(B, i32), entropy=e(B, torch.float32), hnorm=e(B, torch.float32), band=e(B, i32),
                seq=e(B, torch.int64), mask=torch.empty(B, C_, device=device, dtype=torch.uint8), pos_slot=e(B, i32),
                neg_slot=e(B, i32), pos_born=e(C_ * pos_cap + B, i32), pos_evict=e(C_ * pos_cap + B, i32),
                neg_born=e(C_ * neg_cap + B, i32), neg_evict=e(C_ * neg_cap + B, i32))


def tda_adapt(feats, text, state, update=True, out=None, record=None, **hyper):
    """The training-free dynamic adapter (TDA) for ``feats`` [B, d] (unit rows, B <= 8192) against unit class features
    ``text`` [C, d] and the cache ``state`` (``tda_new_state``): B applications of the sequential rule of include/clipfs.h
    in row order, in at most five launches and without a host synchronisation.  ``update=False`` scores against the
    state as it stands and changes nothing; otherwise ``state`` is updated in place.  Returns (logits [B, C], record): the
    record (``tda_new_record``) holds pred, entropy, hnorm, band, seq, mask, pos_slot / neg_slot (-1: not inserted) and the
    born / evict intervals.  ``out`` may be a column slice (row stride >= C, unit column stride); ``hyper`` overrides
    TDA_DEFAULTS except the capacities, which are read off ``state``."""
    assert feats.dim() == 2 and text.dim() == 2 and feats.shape[1] == text.shape[1], (tuple(feats.shape), tuple(text.shape))
    B, d = feats.shape
    Cn = text.shape[0]
    Sp, Sn = state["pos_keys"].shape[1], state["neg_keys"].shape[1]
    shapes = dict(pos_keys=(Cn, Sp, d), pos_ent=(Cn, Sp), pos_seq=(Cn, Sp), neg_keys=(Cn, Sn, d), neg_ent=(Cn, Sn),
                  neg_seq=(Cn, Sn), neg_mask=(Cn, Sn, Cn), counter=(1,))
    for name, shape in shapes.items():
        t = state[name]
        assert t.is_cuda and t.is_contiguous() and t.dtype == _TDA_STATE_DTYPES[name] and tuple(t.shape) == shape, \
            f"tda_adapt: state[{name!r}] must be a contiguous {_TDA_STATE_DTYPES[name]} device tensor of shape {shape}"
    params = tda_params(Cn, d, pos_cap=Sp, neg_cap=Sn, **hyper)
    if out is None:
        out = torch.empty(B, Cn, device=feats.device, dtype=torch.float32)
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, Cn) and out.stride(1) == 1, "out"
    if record is None:
        record = tda_new_record(Cn, B, Sp, Sn, feats.device)
    st, rec = _lib.TdaState(), _lib.TdaRecord()
    st.struct_size, rec.struct_size = C.sizeof(_lib.TdaState), C.sizeof(_lib.TdaRecord)
    for name in _lib.TDA_STATE_FIELDS:
        setattr(st, name, _p(state[name]) if state[name].numel() else None)
    for name in _lib.TDA_RECORD_FIELDS:
        assert record[name].is_contiguous()
        setattr(rec, name, _p(record[name]))
    check(_lib.load().clipfs_tda_adapt(C.byref(params), _p(_f32(feats)), _p(_f32(text)), C.byref(st), _p(out),
                                       out.stride(0) if B > 1 else max(out.stride(0), Cn), C.byref(rec), B, int(bool(update)),
                                       _stream()), "tda_adapt")
    return out, record


# ------------------------------------------------------------------------------------------------ transductive inference
TRANSDUCT_DEFAULTS = dict(logit_scale=100.0, k=3, init_top=8, lam=1.0, shot_weight=1.0, outer=10, inner=5, n_min=1e-6,
                          var_floor=1e-6)
# outputs, state and work of a fit (struct clipfs_transduct_buffers without its inputs): name -> dtype
_TRANSDUCT_OUT = ("z", "labels", "zs_labels", "mu", "var", "nbr", "w")
_TRANSDUCT_INT = ("labels", "zs_labels", "nbr", "sel", "shot_labels")


def transduct_params(N: int, C_: int, d: int, M: int = 0, knn_chunks: int = 0, **hyper):
    """struct clipfs_transduct_params; ``hyper`` overrides TRANSDUCT_DEFAULTS (unknown names: KeyError).  ``knn_chunks`` 0
    lets the plan choose the column chunks of the kNN walk; the result does not depend on them bit for bit."""
    unknown = sorted(set(hyper) - set(TRANSDUCT_DEFAULTS))
    if unknown:
        raise KeyError(f"transduct_params: unknown hyper-parameter(s) {', '.join(unknown)}")
    h = {**TRANSDUCT_DEFAULTS, **hyper}
    for name in ("k", "init_top", "outer", "inner"):
        h[name] = int(h[name])
    return _lib.new_transduct_params(N=N, C=C_, d=d, M=M, knn_chunks=knn_chunks, **h)


def transduct_plan(N: int, C_: int, d: int, M: int = 0, knn_chunks: int = 0, **hyper):
    """What a fit launches (host-only): launches = 6 + (knn_chunks > 1) + outer (inner + 4) whatever N, C, d and M, launch =
    {name: (grid_x, grid_y, grid_z, block, lds_bytes)}, lds_bytes, knn_chunks, class_chunk, stat_splits, stat_rows and
    the work sizes knn_work_bytes, stat_work_floats, nc_floats."""
    return _lib.transduct_plan(transduct_params(N, C_, d, M, knn_chunks, **hyper))


def transduct_shapes(N: int, C_: int, d: int, M: int = 0, knn_chunks: int = 0, **hyper):
    """{member: (shape, dtype)} of the outputs, state and work of struct clipfs_transduct_buffers for these shapes."""
    plan = transduct_plan(N, C_, d, M, knn_chunks, **hyper)
    h = {**TRANSDUCT_DEFAULTS, **hyper}
    k, m = int(h["k"]), int(h["init_top"])
    f32, i32 = torch.float32, torch.int32
    return dict(z=((N, C_), f32), labels=((N,), i32), zs_labels=((N,), i32), mu=((C_, d), f32), var=((d,), f32),
                nbr=((N, k), i32), w=((N, k), f32), logy=((N, C_), f32), u=((N, C_), f32), z2=((N, C_), f32),
                mup=((C_, d), f32), bias=((C_,), f32), n=((C_,), f32), G=((C_, d), f32), Q=((d,), f32), shot_n=((C_,), f32),
                shot_G=((C_, d), f32), sel=((C_, m), i32), stat_work=((plan["stat_work_floats"],), f32),
                knn_work=((plan["knn_work_bytes"] // 4,), f32))


def transduct_buffers(N: int, C_: int, d: int, device, M: int = 0, knn_chunks: int = 0, **hyper):
    """Uninitialised device tensors for every output, state and work member of a fit: every element is written by the fit
    before it is read."""
    return {name: torch.empty(shape, device=device, dtype=dt)
            for name, (shape, dt) in transduct_shapes(N, C_, d, M, knn_chunks, **hyper).items()}


def _transduct_members(**tensors):
    """struct clipfs_transduct_buffers from the named tensors (None and empty tensors stay NULL)."""
    mem = {}
    for name, t in tensors.items():
        if t is None or t.numel() == 0:
            continue
        want = torch.int32 if name in _TRANSDUCT_INT else torch.float32
        assert t.is_cuda and t.is_contiguous() and t.dtype == want, f"transduct: {name} must be a contiguous {want} device tensor"
        mem[name] = t.data_ptr()
    return _lib.new_transduct_buffers(**mem)


def _transduct_shots(shots, shot_labels, d, device):
    """(shots [M, d] or None, device labels or None, host labels or None, M).  Labels given on the host are checked for
    range by the entry point before anything is enqueued; device labels are passed as they are (no host round trip)."""
    if shots is None or shots.shape[0] == 0:
        return None, None, None, 0
    assert shots.dim() == 2 and shots.shape[1] == d and shot_labels is not None and shot_labels.numel() == shots.shape[0], \
        "transduct: shots [M, d] need shot_labels [M]"
    host = None
    if not shot_labels.is_cuda:
        host = shot_labels.to(torch.int32).contiguous()
        dev_labels = host.to(device)
    else:
        dev_labels = shot_labels.to(torch.int32).contiguous()
    return _f32(shots), dev_labels, host, int(shots.shape[0])


def transduct_logy(feats, text, logit_scale=TRANSDUCT_DEFAULTS["logit_scale"]):
    """Step 1 of the rule: (logy [N, C] = log_softmax(s F T^T), zero-shot labels [N] int32, z0 = exp(logy))."""
    (N, d), Cn = feats.shape, text.shape[0]
    params = transduct_params(N, Cn, d, k=1, init_top=1, logit_scale=logit_scale)
    logy, z = torch.empty(N, Cn, device=feats.device), torch.empty(N, Cn, device=feats.device)
    zs = torch.empty(N, device=feats.device, dtype=torch.int32)
    b = _transduct_members(feats=_f32(feats), text=_f32(text), logy=logy, z=z, zs_labels=zs)
    check(_lib.load().clipfs_transduct_logy(C.byref(params), C.byref(b), _stream()), "transduct_logy")
    return logy, zs, z


def transduct_knn(feats, k=TRANSDUCT_DEFAULTS["k"], knn_chunks=0, work=None):
    """Step 2: (nbr [N, k] int32, w [N, k]) -- per row the k most similar OTHER rows, descending, ties to the lower index.
    The N x N similarities never reach memory; ``knn_chunks`` forces the column chunks (the result is bitwise the same);
    ``work``: plan["knn_work_bytes"] // 4 floats, used only with more than one chunk."""
    N, d = feats.shape
    params = transduct_params(N, 1, d, k=k, init_top=1, knn_chunks=knn_chunks)
    plan = _lib.transduct_plan(params)
    if work is None:
        work = torch.empty(plan["knn_work_bytes"] // 4, device=feats.device, dtype=torch.float32)
    assert work.numel() * 4 >= plan["knn_work_bytes"], "transduct_knn: work is too small"
    nbr = torch.empty(N, k, device=feats.device, dtype=torch.int32)
    w = torch.empty(N, k, device=feats.device, dtype=torch.float32)
    b = _transduct_members(feats=_f32(feats), nbr=nbr, w=w, knn_work=work)
    check(_lib.load().clipfs_transduct_knn(C.byref(params), C.byref(b), _stream()), "transduct_knn")
    return nbr, w


def transduct_init(feats, logy, shots=None, shot_labels=None, init_top=TRANSDUCT_DEFAULTS["init_top"],
                   shot_weight=TRANSDUCT_DEFAULTS["shot_weight"]):
    """Step 3 and the shots' constants: dict(sel [C, m] int32 = the m rows of largest logy per class in rank order, mu, mup =
    mu / var, var = 1 / d, shot_n = gamma M_c, shot_G = gamma sum of a class's shots, Q)."""
    (N, d), Cn = feats.shape, logy.shape[1]
    S, y, yh, M = _transduct_shots(shots, shot_labels, d, feats.device)
    params = transduct_params(N, Cn, d, M, k=1, init_top=init_top, shot_weight=shot_weight)
    e = lambda *s: torch.empty(*s, device=feats.device, dtype=torch.float32)
    out = dict(sel=torch.empty(Cn, init_top, device=feats.device, dtype=torch.int32), mu=e(Cn, d), mup=e(Cn, d), var=e(d),
               shot_n=e(Cn), shot_G=e(Cn, d), Q=e(d))
    b = _transduct_members(feats=_f32(feats), logy=_f32(logy), shots=S, shot_labels=y, **out)
    if yh is not None:
        b.shot_labels_host = yh.data_ptr()
    check(_lib.load().clipfs_transduct_init(C.byref(params), C.byref(b), _stream()), "transduct_init")
    return out


def transduct_u(feats, logy, mu, mup, lam=TRANSDUCT_DEFAULTS["lam"]):
    """Step 4.1: (u [N, C] = lam logy + F mup^T + bias, bias [C] = -1/2 sum_d mu mup)."""
    (N, d), Cn = feats.shape, logy.shape[1]
    params = transduct_params(N, Cn, d, k=1, init_top=1, lam=lam)
    u, bias = torch.empty(N, Cn, device=feats.device), torch.empty(Cn, device=feats.device)
    b = _transduct_members(feats=_f32(feats), logy=_f32(logy), mu=_f32(mu), mup=_f32(mup), u=u, bias=bias)
    check(_lib.load().clipfs_transduct_u(C.byref(params), C.byref(b), _stream()), "transduct_u")
    return u, bias


def transduct_z_step(u, nbr, w, z_in, want_labels=False, out=None):
    """Step 4.2, one Jacobi sweep: z_out[i] = softmax(u[i] + sum_r w[i, r] z_in[nbr[i, r]]).  Returns z_out, or (z_out,
    labels [N] int32 = argmax, ties low) with ``want_labels``.  ``out`` must not be ``z_in``."""
    N, Cn = u.shape
    k = nbr.shape[1]
    params = transduct_params(N, Cn, 4, k=k, init_top=1)
    if out is None:
        out = torch.empty(N, Cn, device=u.device, dtype=torch.float32)
    labels = torch.empty(N, device=u.device, dtype=torch.int32) if want_labels else None
    b = _transduct_members(u=_f32(u), nbr=nbr, w=_f32(w))
    check(_lib.load().clipfs_transduct_z_step(C.byref(params), C.byref(b), _p(_f32(z_in)), _p(_f32(out)), _p(labels),
                                              _stream()), "transduct_z_step")
    return (out, labels) if want_labels else out


def transduct_stats(feats, z, mu, shot_n, shot_G, Q, M=0, shot_weight=TRANSDUCT_DEFAULTS["shot_weight"],
                    n_min=TRANSDUCT_DEFAULTS["n_min"], var_floor=TRANSDUCT_DEFAULTS["var_floor"], work=None):
    """Steps 4.3 and 4.4 from z [N, C]: dict(n, G, mu (a new tensor: ``mu`` where n_c <= n_min), var, mup = mu / var).
    ``M`` is the number of shots behind shot_n / shot_G / Q (it enters the variance's denominator N + gamma M)."""
    (N, d), Cn = feats.shape, z.shape[1]
    params = transduct_params(N, Cn, d, M, k=1, init_top=1, shot_weight=shot_weight, n_min=n_min, var_floor=var_floor)
    plan = _lib.transduct_plan(params)
    if work is None:
        work = torch.empty(plan["stat_work_floats"], device=feats.device, dtype=torch.float32)
    assert work.numel() >= plan["stat_work_floats"], "transduct_stats: work is too small"
    e = lambda *s: torch.empty(*s, device=feats.device, dtype=torch.float32)
    out = dict(n=e(Cn), G=e(Cn, d), mu=mu.clone(), var=e(d), mup=e(Cn, d))
    b = _transduct_members(feats=_f32(feats), shot_n=_f32(shot_n), shot_G=_f32(shot_G), Q=_f32(Q), stat_work=work, **out)
    check(_lib.load().clipfs_transduct_stats(C.byref(params), C.byref(b), _p(_f32(z)), _stream()), "transduct_stats")
    return out


def transduct_fit(feats, text, shots=None, shot_labels=None, knn_chunks=0, buffers=None, **hyper):
    """TransCLIP-style transductive inference (the rule of include/clipfs.h, "TRANSDUCT") over the whole test set
    ``feats`` [N, d] (unit rows) against class features ``text`` [C, d], optionally with labelled ``shots`` [M, d] /
    ``shot_labels`` [M]: 6 + (chunks > 1) + outer (inner + 4) launches on the current stream, no host synchronisation,
    bitwise equal run to run.  Returns the ``buffers`` dict (``transduct_buffers``): z, labels, zs_labels, mu, var, nbr, w
    are the outputs of step 5; the rest is state and work.  ``hyper`` overrides TRANSDUCT_DEFAULTS."""
    assert feats.dim() == 2 and text.dim() == 2 and feats.shape[1] == text.shape[1], (tuple(feats.shape), tuple(text.shape))
    (N, d), Cn = feats.shape, text.shape[0]
    S, y, yh, M = _transduct_shots(shots, shot_labels, d, feats.device)
    params = transduct_params(N, Cn, d, M, knn_chunks, **hyper)
    if buffers is None:
        buffers = transduct_buffers(N, Cn, d, feats.device, M, knn_chunks, **hyper)
    for name, (shape, dt) in transduct_shapes(N, Cn, d, M, knn_chunks, **hyper).items():
        t = buffers[name]
        assert tuple(t.shape) == tuple(shape) and t.dtype == dt, f"transduct_fit: buffers[{name!r}] must be {dt} of shape {shape}"
    b = _transduct_members(feats=_f32(feats), text=_f32(text), shots=S, shot_labels=y, **buffers)
    if yh is not None:
        b.shot_labels_host = yh.data_ptr()
    check(_lib.load().clipfs_transduct_fit(C.byref(params), C.byref(b), _stream()), "transduct_fit")
    return buffers


# ------------------------------------------------------------------------------------------------ SPD factor and solve
def spd_plan(n: int, nrhs: int = 1):
    """What ``spd_factor`` and ``spd_solve`` launch for an n x n system with nrhs right-hand sides (host-only):
    factor_launches = ceil(n / 32), solve_launches = 2, the grids, threads and LDS bytes."""
    return _lib.spd_plan(n, nrhs)


def _spd_matrix(t: torch.Tensor, cols: int, what: str) -> torch.Tensor:
    assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == cols and t.stride(1) == 1, \
        f"{what} must be an fp32 device matrix with {cols} columns of unit stride"
    return t


def _ld(t: torch.Tensor) -> int:
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def spd_factor(a: torch.Tensor, out: Optional[torch.Tensor] = None):
    """Cholesky factor of the symmetric positive definite ``a`` [n, n] (only its lower triangle is read): returns
    (chol, info).  ``chol`` holds L on and below the diagonal and L^T above it; ``info`` is a device int32 [1]: 0, or the
    1-based index of the first pivot that is <= 0 or not finite (read it when you want to know: nothing synchronises
    here).  ``a`` and ``out`` may be column slices (row stride >= n, a multiple of 4); ``out=a`` factors in place."""
    n = a.shape[0]
    _spd_matrix(a, n, "spd_factor: a")
    if out is None:
        out = torch.empty(n, n, device=a.device, dtype=torch.float32)
    _spd_matrix(out, n, "spd_factor: out")
    assert out.shape[0] == n
    info = torch.empty(1, device=a.device, dtype=torch.int32)
    check(_lib.load().clipfs_spd_factor(_p(a), _ld(a), _p(out), _ld(out), n, _p(info), _stream()), "spd_factor")
    return out, info


def spd_solve(chol: torch.Tensor, rhs: torch.Tensor, alpha: float = 1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[i, :] = alpha * A^-1 rhs[i, :] for the rows of ``rhs`` [nrhs, n], from ``chol`` = ``spd_factor(A)[0]``.
    ``out=rhs`` solves in place."""
    n = chol.shape[0]
    _spd_matrix(chol, n, "spd_solve: chol")
    _spd_matrix(rhs, n, "spd_solve: rhs")
    if out is None:
        out = torch.empty(rhs.shape[0], n, device=rhs.device, dtype=torch.float32)
    _spd_matrix(out, n, "spd_solve: out")
    assert out.shape[0] == rhs.shape[0]
    check(_lib.load().clipfs_spd_solve(_p(chol), _ld(chol), n, _p(rhs), _ld(rhs), _p(out), _ld(out), rhs.shape[0], alpha,
                                       _stream()), "spd_solve")
    return out


def spd_panels_plan(n: int, nrhs: int = 1, panel: int = 256):
    """What ``spd_factor_panels`` and ``spd_solve_panels`` launch (host-only): panels, band, the kernel launches and GEMM
    calls of the factor and of the solve and lds_bytes."""
    return _lib.spd_panels_plan(n, nrhs, panel)


def spd_factor_panels(a: torch.Tensor, out: Optional[torch.Tensor] = None, panel: int = 256):
    """``spd_factor`` for n up to 16384, right-looking over panels of ``panel`` columns (a multiple of 32 in [32, 1024]):
    the same arguments, the same (chol, info) with ``info`` the first bad pivot as a global 1-based index.  Call
    ``spd_factor`` for n <= 1024; with n <= panel this IS ``spd_factor``, bit for bit."""
    n = a.shape[0]
    _spd_matrix(a, n, "spd_factor_panels: a")
    if out is None:
        out = torch.empty(n, n, device=a.device, dtype=torch.float32)
    _spd_matrix(out, n, "spd_factor_panels: out")
    assert out.shape[0] == n
    info = torch.empty(1, device=a.device, dtype=torch.int32)
    check(_lib.load().clipfs_spd_factor_panels(_p(a), _ld(a), _p(out), _ld(out), n, panel, _p(info), _stream()),
          "spd_factor_panels")
    return out, info


def spd_solve_panels(chol: torch.Tensor, rhs: torch.Tensor, alpha: float = 1.0, out: Optional[torch.Tensor] = None,
                     panel: int = 256) -> torch.Tensor:
    """``spd_solve`` for n up to 16384 from ``spd_factor_panels(A)[0]`` (``panel`` need not be the factor's); the
    right-hand sides live in ``out``, there is no scratch.  ``out=rhs`` solves in place."""
    n = chol.shape[0]
    _spd_matrix(chol, n, "spd_solve_panels: chol")
    _spd_matrix(rhs, n, "spd_solve_panels: rhs")
    if out is None:
        out = torch.empty(rhs.shape[0], n, device=rhs.device, dtype=torch.float32)
    _spd_matrix(out, n, "spd_solve_panels: out")
    assert out.shape[0] == rhs.shape[0]
    check(_lib.load().clipfs_spd_solve_panels(_p(chol), _ld(chol), n, panel, _p(rhs), _ld(rhs), _p(out), _ld(out), rhs.shape[0],
                                              alpha, _stream()),
          "spd_solve_panels")
    return out


# ------------------------------------------------------------------------------------------------ kernel ridge head
def krr_plan(n: int, C_: int, d: int, B: int = 1, panel: int = 256):
    """What ``krr_fit`` and ``krr_apply`` launch (host-only): n4, panelled, fit_launches, factor_launches, solve_launches,
    tiles_per_wave, class_chunk, the apply's grid, threads and lds_bytes."""
    return _lib.krr_plan(n, C_, d, B, panel)


def _n4(n: int) -> int:
    return (n + 3) // 4 * 4


def krr_system(shots, beta=5.5, lam=1.0, out=None):
    """A [n4, n4] = exp(-beta (1 - S S^T)) + lam I of unit ``shots`` [n, d]; pad rows and columns are the identity."""
    n, d = shots.shape
    if out is None:
        out = torch.empty(_n4(n), _n4(n), device=shots.device, dtype=torch.float32)
    _spd_matrix(out, _n4(n), "krr_system: out")
    check(_lib.load().clipfs_krr_system(_p(_f32(shots)), _p(out), n, d, _ld(out), beta, lam, _stream()), "krr_system")
    return out


def _krr_labels(labels, labels_host, n):
    assert labels.is_cuda and labels.dtype == torch.int32 and labels.is_contiguous() and labels.numel() == n, \
        "krr: labels must be a contiguous int32 device vector [n]"
    if labels_host is not None:
        assert not labels_host.is_cuda and labels_host.dtype == torch.int32 and labels_host.is_contiguous() \
            and labels_host.numel() == n
    return None if labels_host is None else labels_host.data_ptr()


def _krr_base(base, rows, cols, what):
    if base is None:
        return None, 0
    assert base.is_cuda and base.dtype == torch.float32 and tuple(base.shape) == (rows, cols) and base.stride(1) == 1, what
    return _p(base), _ld(base)


def krr_targets(labels, n_classes: int, shot_logits=None, target_scale=1.0, labels_host=None, out=None):
    """Et [C, n4]: Et[c, j] = target_scale [labels[j] == c] - shot_logits[j, c]; ``labels`` int32 [n] in any order,
    ``shot_logits`` [n, C] (a column slice is fine) or None.  ``labels_host`` (a CPU int32 copy) is checked first."""
    n = labels.numel()
    lh = _krr_labels(labels, labels_host, n)
    if out is None:
        out = torch.empty(n_classes, _n4(n), device=labels.device, dtype=torch.float32)
    _spd_matrix(out, _n4(n), "krr_targets: out")
    bp, ldb = _krr_base(shot_logits, n, n_classes, "krr_targets: shot_logits [n, C]")
    check(_lib.load().clipfs_krr_targets(_p(labels), lh, bp, ldb, _p(out), n, n_classes, _ld(out), target_scale, _stream()),
          "krr_targets")
    return out


def krr_apply(features, shots, At, base=None, beta=5.5, out=None):
    """out [B, C] = base + exp(-beta (1 - features shots^T)) At[:, :n]^T in one launch; the [B, n] affinity never reaches
    memory.  ``At`` [C, n4] from ``krr_fit``; ``base`` and ``out`` may be column slices; ``out`` must not alias ``base``."""
    B, d = features.shape
    n = shots.shape[0]
    Cn = At.shape[0]
    assert shots.shape[1] == d
    _spd_matrix(At, _n4(n), "krr_apply: At")
    if out is None:
        out = torch.empty(B, Cn, device=features.device, dtype=torch.float32)
    bp, ldb = _krr_base(base, B, Cn, "krr_apply: base [B, C]")
    op, ldo = _krr_base(out, B, Cn, "krr_apply: out [B, C]")
    check(_lib.load().clipfs_krr_apply(_p(_f32(features)), _p(_f32(shots)), _p(At), _ld(At), bp, ldb, op, ldo, B, n, Cn, d, beta,
                                       _stream()), "krr_apply")
    return out


def krr_shapes(n: int, C_: int):
    """{member: (shape, dtype)} of the outputs of struct clipfs_krr_buffers."""
    n4 = _n4(n)
    f32, i32 = torch.float32, torch.int32
    return dict(A=((n4, n4), f32), chol=((n4, n4), f32), info=((1,), i32), Et=((C_, n4), f32), At=((C_, n4), f32))


def krr_buffers(n: int, C_: int, device):
    """Uninitialised device tensors for every output of a fit: every element is written before it is read."""
    return {name: torch.empty(shape, device=device, dtype=dt) for name, (shape, dt) in krr_shapes(n, C_).items()}


def krr_fit(shots, labels, n_classes: int, shot_logits=None, beta=5.5, lam=1.0, target_scale=1.0, panel=256, labels_host=None,
            buffers=None):
    """System, targets, factor and solve of the rule (include/clipfs.h, "KRR") on the current stream, no host
    synchronisation, bitwise the stages called one by one: ``spd_factor`` / ``spd_solve`` when n4 <= 1024, the panelled
    pair above.  Returns the ``buffers`` dict (``krr_buffers``): A, chol, info, Et, At; ``buffers["chol"]`` may be
    ``buffers["A"]`` (the factor then runs in place) and ``buffers["At"]`` may be ``buffers["Et"]``."""
    n, d = shots.shape
    lh = _krr_labels(labels, labels_host, n)
    if buffers is None:
        buffers = krr_buffers(n, n_classes, shots.device)
    for name, (shape, dt) in krr_shapes(n, n_classes).items():
        t = buffers[name]
        assert t.is_cuda and t.is_contiguous() and tuple(t.shape) == tuple(shape) and t.dtype == dt, \
            f"krr_fit: buffers[{name!r}] must be a contiguous {dt} device tensor of shape {shape}"
    bp, ldb = _krr_base(shot_logits, n, n_classes, "krr_fit: shot_logits [n, C]")
    params = _lib.new_krr_params(n=n, C=n_classes, d=d, panel=panel, beta=beta, lambda_=lam, t=target_scale)
    b = _lib.new_krr_buffers(shots=_p(_f32(shots)), labels=_p(labels), labels_host=lh, base_S=bp, ldbs=ldb, A=_p(buffers["A"]),
                             chol=_p(buffers["chol"]), info=_p(buffers["info"]), Et=_p(buffers["Et"]), At=_p(buffers["At"]))
    check(_lib.load().clipfs_krr_fit(C.byref(params), C.byref(b), _stream()), "krr_fit")
    return buffers


# ------------------------------------------------------------------------------------------------ GDA head
GDA_DEFAULT_ALPHAS = tuple(10.0 ** e for e in range(-4, 5))


def gda_params(M: int, C_: int, d: int, prior: str = "uniform", shrink: float = 1.0):
    """struct clipfs_gda_params; ``prior`` is "uniform" or "empirical"."""
    if prior not in _lib.GDA_PRIORS:
        raise ValueError(f"gda: prior must be one of {_lib.GDA_PRIORS}, not {prior!r}")
    return _lib.new_gda_params(M=M, C=C_, d=d, prior=_lib.GDA_PRIORS.index(prior), shrink=shrink)


def gda_plan(M: int, C_: int, d: int, prior: str = "uniform", shrink: float = 1.0):
    """What a fit launches (host-only): launches = 6 + ceil(d / 32) whatever M and C, Mp, factor_launches, solve_launches,
    the grids, lds_bytes and xt_floats."""
    return _lib.gda_plan(gda_params(M, C_, d, prior, shrink))


def gda_shapes(M: int, C_: int, d: int):
    """{member: (shape, dtype)} of the outputs of struct clipfs_gda_buffers for these shapes."""
    Mp = (M + 31) // 32 * 32
    f32, i32 = torch.float32, torch.int32
    return dict(mu=((C_, d), f32), xt=((d, Mp), f32), gram=((d, d), f32), tau=((1,), f32), chol=((d, d), f32),
                info=((1,), i32), W=((C_, d), f32), b=((C_,), f32))


def gda_buffers(M: int, C_: int, d: int, device):
    """Uninitialised device tensors for every output of a fit: every element is written before it is read."""
    return {name: torch.empty(shape, device=device, dtype=dt) for name, (shape, dt) in gda_shapes(M, C_, d).items()}


def _gda_members(offsets_host=None, **tensors):
    mem = {}
    for name, t in tensors.items():
        want = torch.int32 if name in ("offsets", "info") else torch.float32
        assert t.is_cuda and t.is_contiguous() and t.dtype == want, f"gda: {name} must be a contiguous {want} device tensor"
        mem[name] = t.data_ptr()
    b = _lib.new_gda_buffers(**mem)
    if offsets_host is not None:
        assert not offsets_host.is_cuda and offsets_host.dtype == torch.int32 and offsets_host.is_contiguous()
        b.offsets_host = offsets_host.data_ptr()
    return b


def _gda_dims(shots, offsets):
    assert shots.dim() == 2 and offsets.dim() == 1 and offsets.dtype == torch.int32, "gda: shots [M, d], offsets int32 [C + 1]"
    return shots.shape[0], offsets.numel() - 1, shots.shape[1]


def gda_stats(shots, offsets, offsets_host=None):
    """Steps 1 and 2 of the rule (include/clipfs.h, "GDA"): (mu [C, d], xt [d, Mp]) of ``shots`` [M, d] sorted by class with
    ``offsets`` int32 [C + 1].  ``offsets_host`` (a CPU int32 copy) is checked before anything is enqueued."""
    M, Cn, d = _gda_dims(shots, offsets)
    params = gda_params(M, Cn, d)
    sh = gda_shapes(M, Cn, d)
    out = {k: torch.empty(sh[k][0], device=shots.device, dtype=sh[k][1]) for k in ("mu", "xt")}
    b = _gda_members(offsets_host, shots=_f32(shots), offsets=offsets, **out)
    check(_lib.load().clipfs_gda_stats(C.byref(params), C.byref(b), _stream()), "gda_stats")
    return out["mu"], out["xt"]


def gda_shrink(gram, M: int, shrink: float = 1.0):
    """Step 4, in place on ``gram`` [d, d]: adds shrink * trace / (M - 1) to its diagonal; returns (gram, tau [1])."""
    d = gram.shape[0]
    params = gda_params(M, 1, d, shrink=shrink)
    tau = torch.empty(1, device=gram.device, dtype=torch.float32)
    b = _gda_members(gram=_f32(gram), tau=tau)
    check(_lib.load().clipfs_gda_shrink(C.byref(params), C.byref(b), _stream()), "gda_shrink")
    return gram, tau


def gda_bias(mu, W, offsets, M: int, prior: str = "uniform", offsets_host=None):
    """Step 6: b [C] = log pi_c - 1/2 mu_c . W_c."""
    Cn, d = mu.shape
    params = gda_params(M, Cn, d, prior)
    out = torch.empty(Cn, device=mu.device, dtype=torch.float32)
    b = _gda_members(offsets_host, mu=_f32(mu), W=_f32(W), offsets=offsets, b=out)
    check(_lib.load().clipfs_gda_bias(C.byref(params), C.byref(b), _stream()), "gda_bias")
    return out


def gda_search(g, base, target, alphas):
    """hits int32 [nA]: per alpha the rows of ``g`` [B, C] whose argmax_c (base + alpha g), ties to the lower class, equals
    ``target`` (int64 [B]); one launch.  ``base`` [B, C] may be None (0) or a column slice; ``alphas`` is an fp32 device
    vector."""
    B, Cn = g.shape
    assert target.dtype == torch.int64 and target.is_contiguous() and target.numel() == B and target.is_cuda
    assert base is None or (base.dtype == torch.float32 and tuple(base.shape) == (B, Cn) and base.stride(1) == 1)
    hits = torch.empty(alphas.numel(), device=g.device, dtype=torch.int32)
    check(_lib.load().clipfs_gda_search(_p(_f32(g)), _p(base), 0 if base is None else _ld(base), _p(target), _p(_f32(alphas)),
                                        _p(hits), B, Cn, alphas.numel(), _stream()), "gda_search")
    return hits


def gda_fit(shots, offsets, prior: str = "uniform", shrink: float = 1.0, offsets_host=None, buffers=None):
    """Steps 1-6 of the rule on the current stream, 6 + ceil(d / 32) launches, no host synchronisation, bitwise equal run
    to run and bitwise the stages called one by one.  Returns the ``buffers`` dict (``gda_buffers``): mu, xt, gram (after
    the shrinkage), tau, chol, info, W, b."""
    M, Cn, d = _gda_dims(shots, offsets)
    params = gda_params(M, Cn, d, prior, shrink)
    if buffers is None:
        buffers = gda_buffers(M, Cn, d, shots.device)
    for name, (shape, dt) in gda_shapes(M, Cn, d).items():
        t = buffers[name]
        assert tuple(t.shape) == tuple(shape) and t.dtype == dt, f"gda_fit: buffers[{name!r}] must be {dt} of shape {shape}"
    b = _gda_members(offsets_host, shots=_f32(shots), offsets=offsets, **buffers)
    check(_lib.load().clipfs_gda_fit(C.byref(params), C.byref(b), _stream()), "gda_fit")
    return buffers


# ------------------------------------------------------------------------------------------------ contrastive objective
def contrastive_plan(op: str, R: int, N: int, d: int):
    """What ``contrastive_objective`` launches for these shapes ("stats", "combine", "dq", "dk"; host-only): grid, block,
    lds_bytes, col_chunk, chunks, feat_chunk, work_floats."""
    return _lib.contrastive_plan(op, R, N, d)


def contrastive_objective(q, k, q_group, k_group, logit_scale=100.0, weight=1.0, scale_state=None, dq=None, dk=None,
                          want_dq=True, want_dk=True, *, accumulate=True):
    """The one-directional multi-positive InfoNCE loss of unit queries ``q`` [R, d] against unit keys ``k`` [N, d] with
    int32 group ids (a key whose group equals the query's is a positive; a negative key group masks the key out, a
    negative query group or a query without positives contributes nothing): at most four launches, the [R, N] logits and
    their gradient never reach memory.  Returns (loss_sum [1] = weight * sum of the row losses, loss_rows [R], correct [1]
    int32, dq [R, d] or None, dk [N, d] or None).  A passed ``dq`` / ``dk`` is ACCUMULATED into (bitwise old + fresh) and
    returned (``accumulate=False``, or a (dq, dk) pair of flags: overwritten instead); otherwise the gradient is made
    when ``want_dq`` / ``want_dk``.  ``scale_state`` (a loss-scaling record) multiplies the gradients only."""
    R, d = q.shape
    N = k.shape[0]
    assert k.shape[1] == d, (tuple(q.shape), tuple(k.shape))
    for g, n in ((q_group, R), (k_group, N)):
        assert g.dtype == torch.int32 and g.is_contiguous() and g.numel() == n, "groups are contiguous int32 [R] / [N]"
    dev = q.device
    acc_q, acc_k = accumulate if isinstance(accumulate, tuple) else (accumulate, accumulate)
    acc_q, acc_k = acc_q and dq is not None, acc_k and dk is not None
    if dq is None and want_dq:
        dq = torch.empty(R, d, device=dev, dtype=torch.float32)
    if dk is None and want_dk:
        dk = torch.empty(N, d, device=dev, dtype=torch.float32)
    assert dq is None or tuple(dq.shape) == (R, d), "dq is [R, d]"
    assert dk is None or tuple(dk.shape) == (N, d), "dk is [N, d]"
    lib = _lib.load()
    work = torch.empty(_lib.contrastive_plan("stats", R, N, d)["work_floats"], device=dev, dtype=torch.float32)
    loss_rows = torch.empty(R, device=dev, dtype=torch.float32)
    loss_sum = torch.empty(1, device=dev, dtype=torch.float32)
    correct = torch.empty(1, device=dev, dtype=torch.int32)
    check(lib.clipfs_contrastive_objective(_p(_f32(q)), _p(_f32(k)), _p(q_group), _p(k_group), logit_scale, weight,
                                           None if scale_state is None else _p(_scaler(scale_state)), _p(loss_rows),
                                           _p(loss_sum), _p(correct), None if dq is None else _p(_f32(dq)), int(acc_q),
                                           None if dk is None else _p(_f32(dk)), int(acc_k), _p(work), R, N, d, _stream()),
          "contrastive_objective")
    return loss_sum, loss_rows, correct, dq, dk


class ClipLossFn(torch.autograd.Function):
    """``clip_loss``: both directions of the symmetric loss are calls of ``contrastive_objective``; the second call
    accumulates into the first one's gradients."""

    @staticmethod
    def forward(ctx, img, txt, img_group, txt_group, logit_scale):
        img, txt = img.contiguous(), txt.contiguous()
        B, M = img.shape[0], txt.shape[0]
        need_i, need_t = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        l_it, _, _, dimg, dtxt = contrastive_objective(img, txt, img_group, txt_group, logit_scale, 0.5 / B,
                                                       want_dq=need_i, want_dk=need_t)
        l_ti, _, _, dtxt, dimg = contrastive_objective(txt, img, txt_group, img_group, logit_scale, 0.5 / M, dq=dtxt, dk=dimg,
                                                       want_dq=False, want_dk=False)
        ctx.save_for_backward(*(t for t in (dimg, dtxt) if t is not None))
        ctx.have = (dimg is not None, dtxt is not None)
        return (l_it + l_ti).reshape(())

    @staticmethod
    def backward(ctx, dloss):
        saved = list(ctx.saved_tensors)
        dimg = saved.pop(0) * dloss if ctx.have[0] else None
        dtxt = saved.pop(0) * dloss if ctx.have[1] else None
        return dimg, dtxt, None, None, None


def clip_loss(img, txt, img_group=None, txt_group=None, logit_scale=100.0):
    """CLIP's symmetric contrastive loss of unit image rows ``img`` [B, d] and unit caption rows ``txt`` [M, d], a scalar
    with autograd: 1/2 (mean over images of the image -> text loss + mean over captions of the text -> image loss), every
    caption whose group equals an image's being its positive (``contrastive_objective``).  With both groups None the rows
    are pairs (M == B, group = row index).  The means divide by B and M, not by the number of rows that have a positive."""
    if img_group is None and txt_group is None:
        if img.shape[0] != txt.shape[0]:
            raise ValueError(f"clip_loss without groups pairs row i with row i: {img.shape[0]} images, {txt.shape[0]} captions")
        img_group = txt_group = torch.arange(img.shape[0], device=img.device, dtype=torch.int32)
    elif img_group is None or txt_group is None:
        raise ValueError("clip_loss needs both img_group and txt_group, or neither")
    return ClipLossFn.apply(img, txt, img_group.to(torch.int32).contiguous(), txt_group.to(torch.int32).contiguous(),
                            float(logit_scale))


# ---------------------------------------------------------------------------------------------------- sigmoid objective
def sigmoid_plan(op: str, R: int, N: int, d: int):
    """What ``sigmoid_objective`` launches for these shapes ("rows", "combine", "dq", "dk"; host-only): grid, block,
    lds_bytes, feat_chunk.  There is no scratch size: the entry point takes none."""
    return _lib.sigmoid_plan(op, R, N, d)


def sigmoid_objective(q, k, q_group, k_group, head, weight=1.0, scale_state=None, dq=None, dk=None, dhead=None, want_dq=True,
                      want_dk=True, want_dhead=True, accumulate=True):
    """The pairwise sigmoid (SigLIP) loss of unit queries ``q`` [R, d] against unit keys ``k`` [N, d] with int32 group ids
    (a cell whose two groups are equal is a positive, a negative group on either side takes the cell out; a live query
    without a positive still pays its negative terms, unlike ``contrastive_objective``): at most four launches, the
    [R, N] logits and their gradient never reach memory.  ``head``: a DEVICE tensor of two floats (log t, b), read by the
    kernels (nothing passes through the host).  Returns (loss_sum [1] = weight * sum of the cell losses, row_stats [4, R]
    (row loss, sum of sigmoid - [pos], the same times q . k, best live key index as int32 bits), correct [1] int32,
    dq [R, d] or None, dk [N, d] or None, dhead [2] = d / d (log t, b) or None).  A passed ``dq`` / ``dk`` / ``dhead`` is
    ACCUMULATED into (bitwise old + fresh) and returned (``accumulate=False``, or a (dq, dk, dhead) triple of flags:
    overwritten instead); otherwise the gradient is made when ``want_dq`` / ``want_dk`` / ``want_dhead``.
    ``scale_state`` (a loss-scaling record) multiplies the three gradients only."""
    R, d = q.shape
    N = k.shape[0]
    assert k.shape[1] == d, (tuple(q.shape), tuple(k.shape))
    for g, n in ((q_group, R), (k_group, N)):
        assert g.dtype == torch.int32 and g.is_contiguous() and g.numel() == n, "groups are contiguous int32 [R] / [N]"
    assert head.dtype == torch.float32 and head.numel() == 2 and head.is_contiguous(), "head is two contiguous floats (log t, b)"
    dev = q.device
    acc_q, acc_k, acc_h = accumulate if isinstance(accumulate, tuple) else (accumulate,) * 3
    acc_q, acc_k, acc_h = acc_q and dq is not None, acc_k and dk is not None, acc_h and dhead is not None
    if dq is None and want_dq:
        dq = torch.empty(R, d, device=dev, dtype=torch.float32)
    if dk is None and want_dk:
        dk = torch.empty(N, d, device=dev, dtype=torch.float32)
    if dhead is None and want_dhead:
        dhead = torch.empty(2, device=dev, dtype=torch.float32)
    assert dq is None or tuple(dq.shape) == (R, d), "dq is [R, d]"
    assert dk is None or tuple(dk.shape) == (N, d), "dk is [N, d]"
    assert dhead is None or (dhead.numel() == 2 and dhead.is_contiguous()), "dhead is two contiguous floats"
    lib = _lib.load()
    row_stats = torch.empty(4, R, device=dev, dtype=torch.float32)
    loss_sum = torch.empty(1, device=dev, dtype=torch.float32)
    correct = torch.empty(1, device=dev, dtype=torch.int32)
    check(lib.clipfs_sigmoid_objective(_p(_f32(q)), _p(_f32(k)), _p(q_group), _p(k_group), _p(_f32(head)), weight,
                                       None if scale_state is None else _p(_scaler(scale_state)), _p(row_stats), _p(loss_sum),
                                       _p(correct), None if dq is None else _p(_f32(dq)), int(acc_q),
                                       None if dk is None else _p(_f32(dk)), int(acc_k),
                                       None if dhead is None else _p(_f32(dhead)), int(acc_h), R, N, d, _stream()),
          "sigmoid_objective")
    return loss_sum, row_stats, correct, dq, dk, dhead


class SiglipLossFn(torch.autograd.Function):
    """``siglip_loss``: one call of ``sigmoid_objective`` serves both directions."""

    @staticmethod
    def forward(ctx, img, txt, head, img_group, txt_group):
        img, txt, head = img.contiguous(), txt.contiguous(), head.contiguous()
        need = ctx.needs_input_grad[:3]
        loss, _, _, dimg, dtxt, dhead = sigmoid_objective(img, txt, img_group, txt_group, head, 1.0 / img.shape[0],
                                                          want_dq=need[0], want_dk=need[1], want_dhead=need[2])
        ctx.save_for_backward(*(t for t in (dimg, dtxt, dhead) if t is not None))
        ctx.have = (dimg is not None, dtxt is not None, dhead is not None)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, dloss):
        saved = list(ctx.saved_tensors)
        return (*(saved.pop(0) * dloss if have else None for have in ctx.have), None, None)


def siglip_loss(img, txt, img_group=None, txt_group=None, *, head):
    """The sigmoid (SigLIP) loss of unit image rows ``img`` [B, d] and unit caption rows ``txt`` [M, d], a scalar with
    autograd to ``img``, ``txt`` and ``head``: (1/B) sum over all live (image, caption) cells of the binary loss of
    ``sigmoid_objective``, a cell being positive where the two groups are equal.  ``head``: a device tensor of two floats
    (log t, b) (SigLIP starts at t = 10, b = -10).  With both groups None the rows are pairs (M == B, group = row
    index)."""
    if img_group is None and txt_group is None:
        if img.shape[0] != txt.shape[0]:
            raise ValueError(f"siglip_loss without groups pairs row i with row i: {img.shape[0]} images, {txt.shape[0]} captions")
        img_group = txt_group = torch.arange(img.shape[0], device=img.device, dtype=torch.int32)
    elif img_group is None or txt_group is None:
        raise ValueError("siglip_loss needs both img_group and txt_group, or neither")
    return SiglipLossFn.apply(img, txt, head, img_group.to(torch.int32).contiguous(), txt_group.to(torch.int32).contiguous())


# ------------------------------------------------------------------------------------------------- clip pairs objective
def clip_pairs_plan(op: str, R: int, N: int, d: int, both: bool = True):
    """What ``clip_pairs_objective`` launches for these shapes ("rows", "combine", "dq", "dk"; host-only; ``both``:
    weight_k != 0): grid, block, lds_bytes, feat_chunk.  There is no scratch size: the entry point takes none."""
    return _lib.clip_pairs_plan(op, R, N, d, both)


def clip_pairs_objective(q, k, q_group, k_group, head, weight_q, weight_k=0.0, scale_state=None, dq=None, dk=None, dhead=None,
                         want_dq=True, want_dk=True, want_dhead=True, accumulate=False):
    """CLIP's symmetric pair loss in one call, the logit scale on the device: ``contrastive_objective`` of ``q`` [R, d]
    against ``k`` [N, d] with weight ``weight_q`` PLUS the same with the roles swapped and weight ``weight_k``, both at
    s = exp(head[0]); at most four launches, one walk of the logits per gradient carrying both directions.  ``head``: a
    DEVICE tensor of one float, log s, read by the kernels (nothing passes through the host).  ``weight_k == 0``: the
    second direction does not exist (no key statistics; the one-directional call of a data-parallel rank).  Returns
    (loss_sum [1], q_stats [5, R], k_stats [5, N] or None, correct [2] int32 (q -> k, k -> q), dq [R, d] or None,
    dk [N, d] or None, dhead [1] = d loss / d log s or None); a statistics array holds per row lse, 1 / n, the row loss,
    E_softmax[z] - mean_P z and the best live index of the other side as int32 bits.  A passed ``dq`` / ``dk`` / ``dhead``
    is overwritten and returned (``accumulate=True``, or a (dq, dk, dhead) triple of flags: ACCUMULATED into instead,
    bitwise old + fresh); otherwise the gradient is made when ``want_dq`` / ``want_dk`` / ``want_dhead``.
    ``scale_state`` (a loss-scaling record) multiplies the three gradients only."""
    R, d = q.shape
    N = k.shape[0]
    assert k.shape[1] == d, (tuple(q.shape), tuple(k.shape))
    for g, n in ((q_group, R), (k_group, N)):
        assert g.dtype == torch.int32 and g.is_contiguous() and g.numel() == n, "groups are contiguous int32 [R] / [N]"
    assert head.dtype == torch.float32 and head.numel() == 1 and head.is_contiguous(), "head is one float, log s"
    dev = q.device
    acc_q, acc_k, acc_h = accumulate if isinstance(accumulate, tuple) else (accumulate,) * 3
    acc_q, acc_k, acc_h = acc_q and dq is not None, acc_k and dk is not None, acc_h and dhead is not None
    if dq is None and want_dq:
        dq = torch.empty(R, d, device=dev, dtype=torch.float32)
    if dk is None and want_dk:
        dk = torch.empty(N, d, device=dev, dtype=torch.float32)
    if dhead is None and want_dhead:
        dhead = torch.empty(1, device=dev, dtype=torch.float32)
    assert dq is None or tuple(dq.shape) == (R, d), "dq is [R, d]"
    assert dk is None or tuple(dk.shape) == (N, d), "dk is [N, d]"
    assert dhead is None or (dhead.numel() == 1 and dhead.is_contiguous()), "dhead is one float"
    q_stats = torch.empty(5, R, device=dev, dtype=torch.float32)
    k_stats = torch.empty(5, N, device=dev, dtype=torch.float32) if weight_k != 0.0 else None
    loss_sum = torch.empty(1, device=dev, dtype=torch.float32)
    correct = torch.empty(2, device=dev, dtype=torch.int32)
    check(_lib.load().clipfs_clip_pairs_objective(
        _p(_f32(q)), _p(_f32(k)), _p(q_group), _p(k_group), _p(_f32(head)), weight_q, weight_k,
        None if scale_state is None else _p(_scaler(scale_state)), _p(q_stats), _p(k_stats), _p(loss_sum), _p(correct),
        None if dq is None else _p(_f32(dq)), int(acc_q), None if dk is None else _p(_f32(dk)), int(acc_k),
        None if dhead is None else _p(_f32(dhead)), int(acc_h), R, N, d, _stream()), "clip_pairs_objective")
    return loss_sum, q_stats, k_stats, correct, dq, dk, dhead


class ClipPairsLossFn(torch.autograd.Function):
    """``clip_pairs_loss``: ONE symmetric call of ``clip_pairs_objective``."""

    @staticmethod
    def forward(ctx, img, txt, head, img_group, txt_group):
        img, txt, head = img.contiguous(), txt.contiguous(), head.contiguous()
        need = ctx.needs_input_grad[:3]
        loss, _, _, _, dimg, dtxt, dhead = clip_pairs_objective(img, txt, img_group, txt_group, head, 0.5 / img.shape[0],
                                                                0.5 / txt.shape[0], want_dq=need[0], want_dk=need[1],
                                                                want_dhead=need[2])
        ctx.save_for_backward(*(t for t in (dimg, dtxt, dhead) if t is not None))
        ctx.have = (dimg is not None, dtxt is not None, dhead is not None)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, dloss):
        saved = list(ctx.saved_tensors)
        return (*(saved.pop(0) * dloss if have else None for have in ctx.have), None, None)


def clip_pairs_loss(img, txt, img_group=None, txt_group=None, *, head):
    """``clip_loss`` with a trainable temperature: CLIP's symmetric contrastive loss of unit image rows ``img`` [B, d] and
    unit caption rows ``txt`` [M, d] at the logit scale exp(head[0]), a scalar with autograd to ``img``, ``txt`` and
    ``head`` (a device tensor of one float, log s), from one symmetric call with the weights 0.5 / B and 0.5 / M.  With
    both groups None the rows are pairs (M == B, group = row index)."""
    if img_group is None and txt_group is None:
        if img.shape[0] != txt.shape[0]:
            raise ValueError(f"clip_pairs_loss without groups pairs row i with row i: {img.shape[0]} images, {txt.shape[0]} captions")
        img_group = txt_group = torch.arange(img.shape[0], device=img.device, dtype=torch.int32)
    elif img_group is None or txt_group is None:
        raise ValueError("clip_pairs_loss needs both img_group and txt_group, or neither")
    return ClipPairsLossFn.apply(img, txt, head, img_group.to(torch.int32).contiguous(), txt_group.to(torch.int32).contiguous())


# ------------------------------------------------------------------------------------------------ OT matching (PLOT)
def _ot_shapes(x, p):
    assert x.dim() == 3 and p.dim() == 3 and x.shape[2] == p.shape[2], "ot: x is [B, M, d], p is [C, N, d]"
    return x.shape[0], x.shape[1], p.shape[0], p.shape[1], x.shape[2]


def ot_plan(B: int, M: int, C_: int, N: int, d: int):
    """What ``ot_logits`` and ``ot_bwd`` launch for B images of M local rows against C_ classes of N prompts (host-only):
    fwd_launches = dp_launches = dx_launches = 1, the grids, the class chunk, LDS bytes."""
    return _lib.ot_plan(B, M, C_, N, d)


def ot_logits(x, p, mu=None, nu=None, eps=0.1, iters=100, scale=100.0, out=None):
    """(logits [B, C], u [B, C, M], v [B, C, N]): the optimal-transport matching score of include/clipfs.h ("OT
    matching") for unit rows ``x`` [B, M, d] and ``p`` [C, N, d] in one launch.  ``mu`` [B, M] and ``nu`` [C, N] are the
    marginals (None: uniform).  ``u`` and ``v`` are the Sinkhorn scalings ``ot_bwd`` reads.  ``out`` may be a column slice
    (row stride >= C, unit column stride)."""
    B, M, Cn, N, d = _ot_shapes(x, p)
    assert mu is None or tuple(mu.shape) == (B, M), "ot: mu is [B, M]"
    assert nu is None or tuple(nu.shape) == (Cn, N), "ot: nu is [C, N]"
    if out is None:
        out = torch.empty(B, Cn, device=x.device, dtype=torch.float32)
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, Cn) and out.stride(1) == 1, "ot: out"
    u = torch.empty(B, Cn, M, device=x.device, dtype=torch.float32)
    v = torch.empty(B, Cn, N, device=x.device, dtype=torch.float32)
    check(_lib.load().clipfs_ot_logits(_p(_f32(x)), _p(_f32(p)), _p(None if mu is None else _f32(mu)),
                                       _p(None if nu is None else _f32(nu)), _p(out), _ld(out), _p(u), _p(v), B, M, Cn, N, d,
                                       eps, iters, scale, _stream()), "ot_logits")
    return out, u, v


def ot_bwd(x, p, u, v, dlogits, eps=0.1, scale=100.0, dp=None, dx=None, want_dx=False, accumulate=False):
    """(dp [C, N, d], dx [B, M, d] or None): the gradients of ``ot_logits`` for ``dlogits`` [B, C] with the transport plan
    held constant, one launch each.  ``dp`` / ``dx`` given: written, or added to with ``accumulate``; ``dx`` is computed
    when given or ``want_dx``."""
    B, M, Cn, N, d = _ot_shapes(x, p)
    assert tuple(u.shape) == (B, Cn, M) and tuple(v.shape) == (B, Cn, N), "ot: u is [B, C, M], v is [B, C, N]"
    assert dlogits.dtype == torch.float32 and tuple(dlogits.shape) == (B, Cn) and dlogits.stride(1) == 1, "ot: dlogits"
    assert not accumulate or (dp is not None and (dx is not None or not want_dx)), "ot: accumulate needs dp (and dx)"
    if dp is None:
        dp = torch.empty_like(p)
    if dx is None and want_dx:
        dx = torch.empty_like(x)
    assert dp.shape == p.shape and (dx is None or dx.shape == x.shape)
    check(_lib.load().clipfs_ot_bwd(_p(_f32(x)), _p(_f32(p)), _p(_f32(u)), _p(_f32(v)), _p(dlogits), _ld(dlogits), _p(_f32(dp)),
                                    _p(None if dx is None else _f32(dx)), B, M, Cn, N, d, eps, scale, int(bool(accumulate)),
                                    _stream()), "ot_bwd")
    return dp, dx


class OtMatchFn(torch.autograd.Function):
    """``ot_logits`` differentiable w.r.t. ``x`` and ``p`` with the transport plan a constant (PLOT's rule)."""

    @staticmethod
    def forward(ctx, x, p, mu, nu, eps, iters, scale):
        x, p = x.contiguous(), p.contiguous()
        mu = None if mu is None else mu.contiguous()
        nu = None if nu is None else nu.contiguous()
        logits, u, v = ot_logits(x, p, mu, nu, eps, iters, scale)
        ctx.save_for_backward(x, p, u, v)
        ctx.eps, ctx.scale = float(eps), float(scale)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        x, p, u, v = ctx.saved_tensors
        dp, dx = ot_bwd(x, p, u, v, dlogits.contiguous(), ctx.eps, ctx.scale, want_dx=ctx.needs_input_grad[0])
        return dx, dp if ctx.needs_input_grad[1] else None, None, None, None, None, None


def ot_match(x, p, mu=None, nu=None, eps=0.1, iters=100, scale=100.0):
    """logits [B, C] = scale * <T, z>: the optimal-transport matching of unit local rows ``x`` [B, M, d] against unit
    prompt rows ``p`` [C, N, d], T from ``iters`` Sinkhorn iterations at ``eps`` between the marginals ``mu`` [B, M] and
    ``nu`` [C, N] (None: uniform).  Autograd reaches ``x`` and ``p`` only, with T held constant."""
    return OtMatchFn.apply(x, p, mu, nu, eps, iters, scale)
