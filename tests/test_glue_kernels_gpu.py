"""Kernel-level parity of the glue kernels between the GEMMs and the attention: the fp16 storage mode's LayerNorm / row
copies / conversion (norm.hip, elem.hip, gemm_bf16.hip) and the packed-row helpers of the text tower, each called
directly through the C ABI.  Copies, conversions and "two entry points, same arithmetic" comparisons are bit for bit;
everything else is compared with an fp64 torch restatement (oracle/clip_oracle.py) on the same seeded inputs.

Tolerances are those of tests/test_kernels_gpu.py for the same kernel.  Where a shape cannot fit one for a reason that
lies in fp32 itself, the bound is 4 x the error of a float32 CPU restatement against fp64 on the same inputs (``_tol``);
the factor covers the different summation order of the kernel.  No bound is taken from what a kernel produced."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5   # pre-fill of fp32 outputs: what a kernel must not touch keeps it
SENTINEL16 = -1234.0  # the same for f16 buffers (exact in f16)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def _err(got, want):
    return (got.detach().double().cpu() - want.detach().double().cpu()).abs().max().item()


def _close(got, want, atol, what=""):
    err = _err(got, want)
    print(f"{what}: max abs err {err:.3e} (bound {atol:.3e})")
    assert err <= atol, f"{what}: max abs err {err:.3e} > {atol:.3e}"
    return err


def _leaf(t, dt):
    """a fresh autograd leaf holding t's values in dtype dt, on the CPU"""
    return t.detach().cpu().to(dt).clone().requires_grad_()


def _tol(existing, ref32, want64):
    """The kernel's existing tolerance, or 4 x the error of the float32 CPU restatement ``ref32`` against the fp64
    reference where that is larger (a shape whose fp32 rounding alone does not fit the existing figure)."""
    return max(existing, 4.0 * _err(ref32, want64))


def _ptr(t):
    return None if t is None else t.data_ptr()


def _raw(name, *args):
    """status of a C ABI call on the current stream"""
    from clipfs import _lib
    return getattr(_lib.load(), name)(*args, torch.cuda.current_stream().cuda_stream)


def _call(name, *args):
    from clipfs import _lib
    _lib.check(_raw(name, *args), name)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.float16 else t.view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


# ------------------------------------------------------------------ A. fp16 storage mode: LayerNorm with an f16 copy
LN_SHAPES = [(7, 64), (5, 1024), (6, 260), (3, 2048)]  # small; ViT-L/14; nch = 65 (one lane in chunk 2); all 8 chunks


def _ln_case(dev, rows, width, strided):
    """x on the device (class rows of [B, L, d] when strided), its fp64 rows, gamma, beta"""
    if strided:
        full = _rand(rows, 5, width, seed=1)
        x64, ldx = full[:, 0].contiguous(), 5 * width
    else:
        full = _rand(rows, width, seed=1) * 3 + 1
        x64, ldx = full, width
    g, b = 1 + 0.1 * _rand(width, seed=2), _rand(width, seed=3)
    # the references see the fp32 values the kernel sees
    return full.float().to(dev), ldx, x64.float().double(), g.float().double(), b.float().double()


def _ln_fwd_f16(xd, ldx, gd, bd, rows, width, want_y, want_y16):
    y = torch.full((rows, width), SENTINEL, device=xd.device) if want_y else None
    y16 = torch.full((rows, width), SENTINEL16, device=xd.device, dtype=torch.float16) if want_y16 else None
    mean, rstd = torch.empty(rows, device=xd.device), torch.empty(rows, device=xd.device)
    _call("clipfs_layernorm_fwd_f16", xd.data_ptr(), ldx, gd.data_ptr(), bd.data_ptr(), _ptr(y), _ptr(y16),
          mean.data_ptr(), rstd.data_ptr(), rows, width, 1e-5)
    return y, y16, mean, rstd


@pytest.mark.parametrize("rows,width,strided", [(r, w, False) for r, w in LN_SHAPES] + [(6, 128, True)])
def test_layernorm_fwd_f16(dev, rows, width, strided):
    """clipfs_layernorm_fwd_f16 in its three modes (y + y16, y16 alone, y alone): the fp32 outputs are the bits of
    clipfs_layernorm_fwd, the f16 copy is y rounded once, and y matches the fp64 LayerNorm."""
    from clipfs import ops
    from oracle import clip_oracle as O
    xd, ldx, x64, g64, b64 = _ln_case(dev, rows, width, strided)
    gd, bd = g64.float().to(dev), b64.float().to(dev)
    y0, m0, r0 = ops.layernorm_fwd(xd, gd, bd, ldx=ldx, rows=rows, save_stats=True)
    want = O.jt_layer_norm(x64, g64, b64)
    ref32 = O.jt_layer_norm(x64.float(), g64.float(), b64.float())
    _close(y0, want, _tol(2e-5, ref32, want), "ln fwd")
    for want_y, want_y16 in ((True, True), (False, True), (True, False)):
        y, y16, mean, rstd = _ln_fwd_f16(xd, ldx, gd, bd, rows, width, want_y, want_y16)
        assert _same_bits(mean, m0) and _same_bits(rstd, r0), (want_y, want_y16)
        if want_y:
            assert _same_bits(y, y0), "fp32 result differs from clipfs_layernorm_fwd"
        if want_y16:
            assert _same_bits(y16, y0.half()), "f16 copy is not y rounded once"


@pytest.mark.parametrize("with_dres", [False, True])
@pytest.mark.parametrize("rows,width", LN_SHAPES)
def test_layernorm_bwd_f16(dev, rows, width, with_dres):
    """clipfs_layernorm_bwd_f16: dx is bitwise clipfs_layernorm_bwd's, dx16 is dx (residual included) rounded once, and dx
    matches fp64 autograd of the LayerNorm plus dres."""
    from clipfs import ops
    from oracle import clip_oracle as O
    xd, ldx, x64, g64, b64 = _ln_case(dev, rows, width, False)
    gd, bd = g64.float().to(dev), b64.float().to(dev)
    dy64 = _rand(rows, width, seed=4).float().double()
    dres64 = _rand(rows, width, seed=5).float().double() if with_dres else None
    dyd = dy64.float().to(dev)
    dresd = dres64.float().to(dev) if with_dres else None
    _, mean, rstd = ops.layernorm_fwd(xd, gd, bd, save_stats=True)
    dx0 = ops.layernorm_bwd(dyd, xd, gd, mean, rstd, dres=dresd)
    dx = torch.full((rows, width), SENTINEL, device=dev)
    dx16 = torch.full((rows, width), SENTINEL16, device=dev, dtype=torch.float16)
    _call("clipfs_layernorm_bwd_f16", dyd.data_ptr(), xd.data_ptr(), ldx, gd.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
          _ptr(dresd), dx.data_ptr(), dx16.data_ptr(), width, rows, width)
    assert _same_bits(dx, dx0)
    assert _same_bits(dx16, dx.half()), "f16 copy is not the finished dx (residual included) rounded once"
    # without the f16 copy the entry point is the plain backward
    dx1 = torch.full((rows, width), SENTINEL, device=dev)
    _call("clipfs_layernorm_bwd_f16", dyd.data_ptr(), xd.data_ptr(), ldx, gd.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
          _ptr(dresd), dx1.data_ptr(), None, width, rows, width)
    assert _same_bits(dx1, dx0)

    def grad(dt):
        x = _leaf(x64, dt)
        O.jt_layer_norm(x, g64.to(dt), b64.to(dt)).backward(dy64.to(dt))
        return x.grad + (dres64.to(dt) if with_dres else 0)
    want = grad(torch.float64)
    _close(dx, want, _tol(5e-5, grad(torch.float32), want), "ln bwd f16 entry")


def test_layernorm_bwd_f16_leading_dimension_and_in_place(dev):
    """dx and dres at lddx = 320 > width = 256: the 64 pad columns keep their sentinel, the written part is the plain
    backward's bits, and the contiguous f16 copy [rows, width] is dx[:, :width] rounded once.  Then the tower's in-place
    form (dres and dx the same buffer), which must give the out-of-place bits."""
    from clipfs import ops
    rows, width, lddx = 6, 256, 320
    xd, ldx, _, g64, b64 = _ln_case(dev, rows, width, False)
    gd, bd = g64.float().to(dev), b64.float().to(dev)
    dyd = _rand(rows, width, seed=4).float().to(dev)
    dres = _rand(rows, lddx, seed=5).float().to(dev)  # pad columns carry data that must not travel
    _, mean, rstd = ops.layernorm_fwd(xd, gd, bd, save_stats=True)
    dx0 = ops.layernorm_bwd(dyd, xd, gd, mean, rstd, dres=dres[:, :width].contiguous())
    dx = torch.full((rows, lddx), SENTINEL, device=dev)
    # the f16 copy is the first rows * width elements of a buffer sized for the WRONG stride, so a copy written at
    # stride lddx stays inside the allocation and shows in the guard part
    buf16 = torch.full((rows * lddx,), SENTINEL16, device=dev, dtype=torch.float16)
    args = (dyd.data_ptr(), xd.data_ptr(), ldx, gd.data_ptr(), mean.data_ptr(), rstd.data_ptr())
    _call("clipfs_layernorm_bwd_f16", *args, dres.data_ptr(), dx.data_ptr(), buf16.data_ptr(), lddx, rows, width)
    assert _same_bits(dx[:, :width].contiguous(), dx0)
    assert (dx[:, width:] == SENTINEL).all(), "pad columns of dx were written"
    assert _same_bits(buf16[:rows * width].view(rows, width), dx[:, :width].contiguous().half())
    assert (buf16[rows * width:] == SENTINEL16).all(), "f16 copy written past [rows, width]"
    # the plain entry point at the same leading dimension
    dx2 = torch.full((rows, lddx), SENTINEL, device=dev)
    ops.layernorm_bwd(dyd, xd, gd, mean, rstd, dres=dres, dx=dx2, lddx=lddx)
    assert _same_bits(dx2, dx)
    # in place
    for ld in (lddx, width):
        res = dres[:, :ld].contiguous()
        out = torch.full((rows, ld), SENTINEL, device=dev)
        out16 = torch.empty(rows, width, device=dev, dtype=torch.float16)
        _call("clipfs_layernorm_bwd_f16", *args, res.data_ptr(), out.data_ptr(), out16.data_ptr(), ld, rows, width)
        inpl = res.clone()
        inpl16 = torch.empty(rows, width, device=dev, dtype=torch.float16)
        _call("clipfs_layernorm_bwd_f16", *args, inpl.data_ptr(), inpl.data_ptr(), inpl16.data_ptr(), ld, rows, width)
        assert _same_bits(inpl[:, :width].contiguous(), out[:, :width].contiguous()) and _same_bits(inpl16, out16)
        assert _same_bits(inpl[:, width:].contiguous(), res[:, width:].contiguous())


# ------------------------------------------------------------------ A. one row per sequence, f16 storage
@pytest.mark.parametrize("n,seq,width,ld", [(37, 11, 20, 28), (4200, 2, 512, 520)])  # 2nd: n * width > 8192 * 256 threads
def test_seq_rows_f16(dev, n, seq, width, ld):
    """clipfs_gather_seq_rows_f16 / clipfs_put_seq_rows_f16: exact widening / one rounding of the indexed rows; every
    other row and the pad columns beyond ``width`` keep their contents."""
    g = torch.Generator().manual_seed(n)
    src16 = (torch.randn(n * seq, ld, generator=g) * 4).half().to(dev)
    idx = torch.randint(0, seq, (n,), generator=g, dtype=torch.int32).to(dev)
    flat = torch.arange(n, device=dev) * seq + idx.long()
    out = torch.full((n, width), SENTINEL, device=dev)
    _call("clipfs_gather_seq_rows_f16", src16.data_ptr(), ld, idx.data_ptr(), out.data_ptr(), n, seq, width)
    assert _same_bits(out, src16[flat, :width].float())
    src = (torch.randn(n, width, generator=g) * 4).to(dev)  # not f16-representable: the put rounds
    dst = (torch.randn(n * seq, ld, generator=g)).half().to(dev)
    want = dst.clone()
    want[flat, :width] = src.half()
    _call("clipfs_put_seq_rows_f16", src.data_ptr(), idx.data_ptr(), dst.data_ptr(), ld, n, seq, width)
    assert _same_bits(dst, want)


# ------------------------------------------------------------------ A. fp32 -> f16 conversion
_PLANTED = [70000.0, -1.0e5, 65519.99, 65520.0,          # above 65 504: inf, -inf, largest finite, tie -> inf
            3.0e-6, -2.0 ** -25, 2.0 ** -24 * 1.5, -0.0,   # f16 subnormals: plain, tie -> -0, tie -> even, signed zero
            1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 6.1e-5, -6.0e-8,  # ties to even (down, up), largest subnormals
            0.1, -3.14159, 1.0e-10, 60000.0]


@pytest.mark.parametrize("n", [8, 8 * 257, 8 * (8192 * 256 + 3)])  # last: second pass of the grid-stride loop (67 MB in)
def test_convert_f16(dev, n):
    """clipfs_convert_f16 bit for bit against .half() (round to nearest even, overflow to inf, subnormals, -0)."""
    from clipfs import ops
    g = torch.Generator().manual_seed(5)
    src = torch.randn(n, generator=g) * 8
    planted = torch.tensor(_PLANTED, dtype=torch.float32)
    if n == 8:
        src[:] = planted[[0, 1, 4, 7, 8, 9, 3, 5]]
    else:
        for at in (0, n // 2 + 3, n - 16):  # start, middle, the tail that only the second pass reaches
            src[at:at + 16] = planted
    out = ops.to_f16(src.to(dev))
    want = src.half()
    assert want.isinf().any() and (want == 0).any()
    assert _same_bits(out.cpu(), want)


def test_convert_f16_refuses_ragged_and_misaligned(dev):
    src = torch.ones(64, device=dev)
    dst = torch.full((64,), SENTINEL16, device=dev, dtype=torch.float16)
    assert _raw("clipfs_convert_f16", src.data_ptr(), dst.data_ptr(), 12) == 1
    assert _raw("clipfs_convert_f16", src.data_ptr() + 4, dst.data_ptr(), 8) == 1
    assert _raw("clipfs_convert_f16", src.data_ptr(), dst.data_ptr() + 4, 8) == 1
    torch.cuda.synchronize()
    assert (dst == SENTINEL16).all(), "a refused call launched something"
    _call("clipfs_convert_f16", src.data_ptr(), dst.data_ptr(), 8)
    assert (dst[:8] == 1).all() and (dst[8:] == SENTINEL16).all()


# ------------------------------------------------------------------ B. packed-row helpers
ROWS_MAP_CASES = [  # n, width, ld, base offset in floats, path
    (53, 512, 512, 0, "vector"),
    (53, 20, 28, 0, "vector"),
    (53, 18, 22, 0, "scalar: width % 4"),
    (53, 20, 22, 0, "scalar: ld % 4"),
    (53, 512, 512, 1, "scalar: base pointer off by one float"),
    (4200, 2048, 2048, 0, "vector, n * width / 4 > 8192 * 256 threads"),
]


@pytest.mark.parametrize("n,width,ld,off,path", ROWS_MAP_CASES)
def test_gather_rows_map(dev, n, width, ld, off, path):
    """out[i, :] = src[map[i], :width] exactly, through a map with repeats and out-of-order rows."""
    g = torch.Generator().manual_seed(width + ld + off)
    nsrc = 97
    store = torch.randn(nsrc * ld + off, generator=g).to(dev)
    src = store[off:].view(nsrc, ld)
    rmap = torch.randint(0, nsrc, (n,), generator=g, dtype=torch.int32)
    rmap[:4] = torch.tensor([96, 0, 96, 5], dtype=torch.int32)
    rmap = rmap.to(dev)
    out = torch.full((n, width), SENTINEL, device=dev)
    _call("clipfs_gather_rows_map", src.data_ptr(), ld, rmap.data_ptr(), out.data_ptr(), n, width)
    assert _same_bits(out, src[rmap.long(), :width].contiguous()), path


@pytest.mark.parametrize("n,width,ld,off,path", ROWS_MAP_CASES)
def test_put_rows_map(dev, n, width, ld, off, path):
    """dst[map[i], :width] = src[i, :] exactly through a map of unique rows; unmapped rows and pad columns keep the sentinel."""
    g = torch.Generator().manual_seed(width + ld + off + 1)
    ndst = n + 44
    store = torch.full((ndst * ld + off,), SENTINEL, device=dev)
    dst = store[off:].view(ndst, ld)
    rmap = torch.randperm(ndst, generator=g)[:n].to(torch.int32).to(dev)
    src = torch.randn(n, width, generator=g).to(dev)
    want = store.clone()
    want[off:].view(ndst, ld)[rmap.long(), :width] = src
    _call("clipfs_put_rows_map", src.data_ptr(), rmap.data_ptr(), dst.data_ptr(), ld, n, width)
    assert _same_bits(store, want), path


@pytest.mark.parametrize("with_dres", [False, True])
@pytest.mark.parametrize("width", [260, 512])
def test_layernorm_bwd_rows(dev, width, with_dres):
    """clipfs_layernorm_bwd_rows reads x, mean and rstd at xmap[row] of the saved full-layout tensors: bitwise the plain
    backward on the gathered rows, and fp64 autograd within tolerance."""
    from clipfs import ops
    from oracle import clip_oracle as O
    rows, saved, ldx = 45, 200, width + 64
    g = torch.Generator().manual_seed(width)
    xs = (torch.randn(saved, ldx, generator=g) * 3 + 1).to(dev)
    g64, b64 = (1 + 0.1 * _rand(width, seed=2)).float().double(), _rand(width, seed=3).float().double()
    gd, bd = g64.float().to(dev), b64.float().to(dev)
    _, mean, rstd = ops.layernorm_fwd(xs, gd, bd, ldx=ldx, rows=saved, save_stats=True)
    xmap = torch.randint(0, saved, (rows,), generator=g, dtype=torch.int32)
    xmap[:5] = torch.tensor([199, 3, 199, 0, 150], dtype=torch.int32)  # repeats, not monotone
    xmap = xmap.to(dev)
    dy = torch.randn(rows, width, generator=g).to(dev)
    dres = torch.randn(rows, width, generator=g).to(dev) if with_dres else None
    dx = torch.full((rows, width), SENTINEL, device=dev)
    _call("clipfs_layernorm_bwd_rows", dy.data_ptr(), xs.data_ptr(), ldx, gd.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
          xmap.data_ptr(), _ptr(dres), dx.data_ptr(), width, rows, width)
    m = xmap.long()
    xg = xs[m, :width].contiguous()
    dx0 = ops.layernorm_bwd(dy, xg, gd, mean[m].contiguous(), rstd[m].contiguous(), dres=dres)
    assert _same_bits(dx, dx0)

    def grad(dt):
        x = _leaf(xg, dt)
        O.jt_layer_norm(x, g64.to(dt), b64.to(dt)).backward(dy.cpu().to(dt))
        return x.grad + (dres.cpu().to(dt) if with_dres else 0)
    want = grad(torch.float64)
    _close(dx, want, _tol(5e-5, grad(torch.float32), want), "ln bwd rows")


@pytest.mark.parametrize("width", [192, 512])
@pytest.mark.parametrize("r", [1, 2, 4])
def test_layernorm_fwd_lora_map(dev, r, width):
    """clipfs_layernorm_fwd_lora_map on packed rows draws the dropout masks of the rows' full-layout positions: y, t and the
    keep bits are bitwise rows drow0 + map[row] of the unmapped kernel run on the full layout with the same seed."""
    full, rows, seed, sb, drow0, p, mask = 61, 23, 0x9E3779B97F4A7C15 >> 1, 5, 1000, 0.25, 0b101
    g = torch.Generator().manual_seed(width + r)
    x = (torch.randn(full, width, generator=g) * 2 + 0.3).to(dev)
    gd = (1 + 0.1 * torch.randn(width, generator=g)).to(dev)
    bd = (0.1 * torch.randn(width, generator=g)).to(dev)
    A = (torch.randn(3 * r, width, generator=g) * width ** -0.5).to(dev)
    rmap = torch.randperm(full, generator=g)[:rows].to(torch.int32)
    rmap[3] = rmap[0]  # a repeat
    rmap = rmap.to(dev)
    nch = width // 4

    def run(xin, n, drow_map):
        y = torch.full((n, width), SENTINEL, device=dev)
        t = torch.full((n, 3 * r), SENTINEL, device=dev)
        mean, rstd = torch.empty(n, device=dev), torch.empty(n, device=dev)
        kb = torch.zeros(n, nch, device=dev, dtype=torch.int16)
        head = (xin.data_ptr(), width, gd.data_ptr(), bd.data_ptr(), y.data_ptr(), None, mean.data_ptr(), rstd.data_ptr(),
                n, width, 1e-5, A.data_ptr(), t.data_ptr(), r, 3, mask, p, seed, sb, drow0)
        if drow_map is None:
            _call("clipfs_layernorm_fwd_lora", *head, kb.data_ptr())
        else:
            _call("clipfs_layernorm_fwd_lora_map", *head, drow_map.data_ptr(), kb.data_ptr())
        return y, t, kb, mean, rstd

    yf, tf, kbf, mf, rf = run(x, full, None)
    m = rmap.long()
    yp, tp, kbp, mp, rp = run(x[m].contiguous(), rows, rmap)
    assert _same_bits(yp, yf[m]) and _same_bits(mp, mf[m]) and _same_bits(rp, rf[m])
    assert torch.equal(kbp, kbf[m]) and kbf.any()
    assert _same_bits(tp, tf[m])
    assert (tp[:, r:2 * r] == 0).all() and (tf[:, r:2 * r] == 0).all(), "the segment that is off must give zeros"
    assert tp[:, :r].abs().min() > 0 and tp[:, 2 * r:].abs().min() > 0
    # the masks depend on the full-layout row: the identity map draws other masks for these rows
    ident = torch.arange(rows, dtype=torch.int32, device=dev)
    _, t_id, kb_id, _, _ = run(x[m].contiguous(), rows, ident)
    assert not torch.equal(kb_id, kbp)
    # segments 0 and 2 occupy bits 0-3 and 8-11 of the keep word, segment 1 (off) none
    assert ((kbp.int() & 0xF0F0) == 0).all()


# ------------------------------------------------------------------ C. cross entropy
CE_SHAPES = [(1, 1), (3, 2), (5, 63), (4, 64), (7, 65), (256, 403), (1001, 1000)]


def _ce_inputs(rows, classes):
    """logits at the workload's scale (100 x cosine: a spread of about +-30), with a row whose target towers 80 above the
    rest, one whose target lies 80 below, and one with two equal maxima (the first is the target)."""
    rs = np.random.RandomState(rows * 1000 + classes)
    z = (_rand(rows, classes, seed=rows + classes) * 10).float()
    tgt = torch.from_numpy(rs.randint(0, classes, rows))
    if rows >= 3 and classes >= 2:
        z[0] = z[0] / 10
        z[0, tgt[0]] = z[0].max() + 80
        t1 = int(tgt[1])
        z[1, t1] = torch.cat([z[1, :t1], z[1, t1 + 1:]]).min() - 80
        a, b = (3, 67) if classes > 67 else (0, classes - 1)
        z[2, a] = z[2, b] = z[2].max() + 1
        tgt[2] = a
    return z, tgt


@pytest.mark.parametrize("rows,classes", CE_SHAPES)
def test_cross_entropy_shapes(dev, rows, classes):
    from clipfs import ops
    from oracle import clip_oracle as O
    z32, tgt = _ce_inputs(rows, classes)
    gs = 0.5

    def ref(dt):
        z = _leaf(z32, dt)
        loss = O.jt_cross_entropy(z, tgt)
        loss.backward()
        return loss.detach().reshape(1), z.grad * gs
    loss64, grad64 = ref(torch.float64)
    loss32, grad32 = ref(torch.float32)
    ls, dl, correct = ops.cross_entropy(z32.to(dev), tgt.to(dev), grad_scale=gs)
    # 1e-5 / 1e-6 are test_kernels_gpu.py's.  A row with a loss near 80 has an fp32 ulp of 8e-6, so _tol would take 4 x
    # the float32 restatement's error if that were larger; measured on the CPU it is not: the restatement's loss is off
    # by at most 2.2e-6 (3 x 2; 1.6e-6 at 4 x 64, 1.2e-6 at 1001 x 1000) -> 8.9e-6, its gradient by 8.3e-9 -> 3.3e-8
    _close(ls / rows, loss64, _tol(1e-5, loss32, loss64), "ce loss")
    _close(dl, grad64, _tol(1e-6, grad32, grad64), "ce grad")
    assert correct.item() == int((z32.argmax(1) == tgt).sum()), "correct must agree with argmax (first maximum wins)"
    ls2, dl2, correct2 = ops.cross_entropy(z32.to(dev), tgt.to(dev), want_grad=False, grad_scale=gs)
    assert dl2 is None and _same_bits(ls2, ls) and correct2.item() == correct.item()


# ------------------------------------------------------------------ C. top-k
@pytest.mark.parametrize("classes,k", [(5, 5), (64, 8), (65, 5), (403, 1), (1000, 5), (70, 70)])
def test_topk_shapes(dev, classes, k):
    """Equal values at c, c + 64 and c + 128 (the same lane's strides), -inf entries and constant rows: exactly O.jt_topk
    (larger value first, then the smaller index) on the same fp32 values."""
    from clipfs import ops
    from oracle import clip_oracle as O
    z = _rand(12, classes, seed=classes + k).float()
    z[0] = 2.5                                         # all equal
    z[1] = float("-inf")                               # all equal at -inf
    for row, c in ((2, 1), (3, 0), (4, classes - 1)):  # the largest value three times, 64 apart (where they exist)
        top = z[row].max() + 1
        for cc in (c, c + 64, c + 128, c - 64, c - 128):
            if 0 <= cc < classes:
                z[row, cc] = top
    z[5, ::2] = float("-inf")                          # -inf at every even class
    z[6, 1:] = float("-inf")                           # one finite entry
    z[7, :-1] = float("-inf")                          # the only finite entry is the last
    z[8] = z[8].round()                                # many ties
    z[9, : classes // 2] = 1.0                         # ties in a block, the rest random
    got = ops.topk(z.to(dev), k).cpu().long()
    assert torch.equal(got, O.jt_topk(z, k))


# ------------------------------------------------------------------ C. class mean, l2norm, LayerNorm at more shapes
@pytest.mark.parametrize("classes,templates,width", [(403, 1, 512), (5, 7, 768), (3, 2, 2048), (4, 3, 200), (2, 1, 4)])
def test_class_mean_shapes(dev, classes, templates, width):
    from clipfs import ops
    from oracle import clip_oracle as O
    emb32 = _rand(classes * templates, width, seed=width + classes).float()
    dout32 = _rand(classes, width, seed=4).float()
    cls_idx = [c for c in range(classes) for _ in range(templates)]

    def ref(dt):
        e = _leaf(emb32, dt)
        out = O.class_text_features(e, cls_idx, classes).t()
        out.backward(dout32.to(dt))
        return out.detach(), e.grad
    out64, g64 = ref(torch.float64)
    out32, g32 = ref(torch.float32)
    _close(ops.class_mean_fwd(emb32.to(dev), classes, templates), out64, _tol(1e-6, out32, out64), "class mean fwd")
    # float32 restatement, measured on the CPU: at most 3.8e-8 forward, 1.0e-7 backward (2 x 1 x 4), so 1e-6 / 1e-5 hold
    _close(ops.class_mean_bwd(emb32.to(dev), dout32.to(dev), classes, templates), g64, _tol(1e-5, g32, g64),
           "class mean bwd")


def test_class_mean_refuses_width_2049(dev):
    from clipfs import ops
    from clipfs._lib import ClipfsError
    emb, dout = torch.ones(2, 2049, device=dev), torch.ones(2, 2049, device=dev)
    with pytest.raises(ClipfsError):
        ops.class_mean_fwd(emb, 2, 1)
    with pytest.raises(ClipfsError):
        ops.class_mean_bwd(emb, dout, 2, 1)


@pytest.mark.parametrize("rows,width", [(1, 4), (403, 512), (130, 768), (5, 2048), (9, 1028)])
def test_l2norm_shapes(dev, rows, width):
    from clipfs import ops
    from oracle import clip_oracle as O
    x32, dy32 = _rand(rows, width, seed=rows).float(), _rand(rows, width, seed=2).float()

    def ref(dt):
        x = _leaf(x32, dt)
        y = O.l2_normalize(x)
        y.backward(dy32.to(dt))
        return y.detach(), x.grad
    y64, g64 = ref(torch.float64)
    y32, g32 = ref(torch.float32)
    yg, inv = ops.l2norm_fwd(x32.to(dev), save_inv=True)
    _close(yg, y64, _tol(1e-6, y32, y64), "l2norm fwd")
    _close(ops.l2norm_bwd(dy32.to(dev), yg, inv), g64, _tol(1e-5, g32, g64), "l2norm bwd")


@pytest.mark.parametrize("width", [4, 200, 260, 1280, 2048])
def test_layernorm_more_widths(dev, width):
    from clipfs import ops
    from oracle import clip_oracle as O
    rows = 9
    xd, ldx, x64, g64, b64 = _ln_case(dev, rows, width, False)
    gd, bd = g64.float().to(dev), b64.float().to(dev)
    dy64, dres64 = _rand(rows, width, seed=4).float().double(), _rand(rows, width, seed=5).float().double()

    def ref(dt):
        x = _leaf(x64, dt)
        y = O.jt_layer_norm(x, g64.to(dt), b64.to(dt))
        y.backward(dy64.to(dt))
        return y.detach(), x.grad + dres64.to(dt)
    y64, dx64 = ref(torch.float64)
    y32, dx32 = ref(torch.float32)
    y, mean, rstd = ops.layernorm_fwd(xd, gd, bd, save_stats=True)
    _close(y, y64, _tol(2e-5, y32, y64), "ln fwd")
    # float32 restatement, measured on the CPU: forward 6.7e-7 and backward 2.1e-7 at width 2048 (the largest of the
    # five), so 4 x that stays under the existing 2e-5 / 5e-5
    dx = ops.layernorm_bwd(dy64.float().to(dev), xd, gd, mean, rstd, dres=dres64.float().to(dev))
    _close(dx, dx64, _tol(5e-5, dx32, dx64), "ln bwd")


@pytest.mark.parametrize("width", [2052, 6])
def test_layernorm_refuses_unsupported_width(dev, width):
    from clipfs import ops
    from clipfs._lib import ClipfsError
    x = torch.ones(4, width, device=dev)
    g = torch.ones(width, device=dev)
    stat = torch.ones(4, device=dev)
    with pytest.raises(ClipfsError):
        ops.layernorm_fwd(x, g, g)
    with pytest.raises(ClipfsError):
        ops.layernorm_bwd(x, x, g, stat, stat)


# ------------------------------------------------------------------ C. logit_normalize
def _logit_normalize_ref(z32, dzn32, dt):
    from oracle import clip_oracle as O
    z = _leaf(z32, dt)
    zn = O.logit_normalize(z)
    zn.backward(dzn32.to(dt))
    return zn.detach(), z.grad


@pytest.mark.parametrize("rows,classes", [(1, 2), (16, 64), (17, 403), (435, 403)])  # last: the stage-2 head's own size
def test_logit_normalize_fwd_bwd(dev, rows, classes):
    from clipfs import ops
    z32 = (_rand(rows, classes, seed=rows) * 3 + 0.5).float()
    dzn32 = _rand(rows, classes, seed=7).float()
    zn64, dz64 = _logit_normalize_ref(z32, dzn32, torch.float64)
    zn32, dz32 = _logit_normalize_ref(z32, dzn32, torch.float32)
    _close(ops.logit_normalize(z32.to(dev)), zn64, _tol(1e-4, zn32, zn64), "logit_normalize")
    # no tolerance existed: 4 x the float32 restatement's error against fp64 (measured on the CPU: 2.0e-7 at 435 x 403
    # -> 8.1e-7, 1.3e-7 at 17 x 403 -> 5.0e-7, 1.1e-7 at 16 x 64 -> 4.6e-7, 8.9e-8 at 1 x 2 -> 3.6e-7)
    _close(ops.logit_normalize_bwd(z32.to(dev), dzn32.to(dev)), dz64, 4 * _err(dz32, dz64), "logit_normalize bwd")


@pytest.mark.parametrize("noise", [0.0, 5e-4])
def test_logit_normalize_bwd_clamped_variance(dev, noise):
    """A constant (or nearly constant) z has a variance under the 1e-6 clamp: sigma is the constant 1e-3 and its term of
    the gradient vanishes, as torch.clamp's zero gradient makes it in O.jt_std.  With noise the unclamped formula's
    sigma term would be of order 1 on a gradient of order 1e3."""
    from clipfs import ops
    rows, classes = 16, 64
    z32 = (2.5 + noise * _rand(rows, classes, seed=3)).float()
    assert z32.double().var().item() < 1e-6
    dzn32 = _rand(rows, classes, seed=7).float()
    _, dz64 = _logit_normalize_ref(z32, dzn32, torch.float64)
    _, dz32 = _logit_normalize_ref(z32, dzn32, torch.float32)
    want = (dzn32.double() - dzn32.double().mean(1, keepdim=True)) / 1e-3  # the sigma term gone
    assert _err(dz64, want) < 1e-9
    # 4 x the float32 restatement's error: entries reach 3.1e3 (one fp32 ulp there is 2.4e-4); measured on the CPU
    # 3.5e-4 -> bound 1.4e-3, for both inputs
    bound = 4 * _err(dz32, dz64)
    _close(ops.logit_normalize_bwd(z32.to(dev), dzn32.to(dev)), dz64, bound, "logit_normalize bwd (clamped)")


# ------------------------------------------------------------------ C. matmul_small, colsum
@pytest.mark.parametrize("M,N,K", [(435, 64, 403), (403, 64, 435), (1, 1, 1)])
@pytest.mark.parametrize("pattern", ["dz @ W", "dz^T @ f"])
def test_matmul_small(dev, M, N, K, pattern):
    """Both stride patterns of the callers with alpha = 100; O(1) results, tolerance of the GEMM tests."""
    from clipfs import ops
    a = _rand(M, K, seed=1).float()
    b = (_rand(K, N, seed=2) * K ** -0.5 / 100).float()
    want = 100.0 * (a.double() @ b.double())
    ref32 = 100.0 * (a @ b)
    if pattern == "dz @ W":
        got = ops.matmul_small(a.to(dev), b.to(dev), M, N, K, K, 1, N, 1, 100.0)
    else:  # A stored as its transpose [K, M]: element (m, k) at m + k * M
        got = ops.matmul_small(a.t().contiguous().to(dev), b.to(dev), M, N, K, 1, M, N, 1, 100.0)
    _close(got, want, _tol(2e-5 * K ** 0.5 * 4, ref32, want), f"matmul_small {pattern}")


@pytest.mark.parametrize("with_y", [False, True])
@pytest.mark.parametrize("rows", [1, 435])
@pytest.mark.parametrize("cols", [1, 255, 256, 257, 403])
def test_colsum(dev, cols, rows, with_y):
    from clipfs import ops
    x32 = _rand(rows, cols, seed=cols + rows).float()
    y32 = _rand(rows, cols, seed=9).float() if with_y else None
    want = (x32.double() * (y32.double() if with_y else 1)).sum(0)
    # float32 restatement in the kernel's fixed row order; with y one rounding per row (a fused multiply-add: the exact
    # product and the sum in fp64, rounded to fp32 once)
    acc = torch.zeros(cols)
    for r in range(rows):
        acc = (acc.double() + x32[r].double() * y32[r].double()).float() if with_y else acc + x32[r]
    # no tolerance existed: 4 x the restatement's error.  Measured on the CPU at 435 rows (sums near 20 - 60): 3.2e-6 for
    # the single column, 3.0e-5 - 4.6e-5 from 255 columns up -> bounds 1.3e-5 and 1.2e-4 - 1.8e-4; one row: 0 without y
    # (a copy), one rounding of the product with y (2.0e-7 -> 7.8e-7)
    got = ops.colsum(x32.to(dev), y32.to(dev) if with_y else None)
    _close(got, want, 4 * _err(acc, want), "colsum")


# ------------------------------------------------------------------ C. AdamW
def _adamw_f32(p, g, m, v, step, lr, b1, b2, eps, wd, gs):
    """float32 restatement in the kernel's order of operations (scalars rounded to fp32 as the C ABI receives them)"""
    f = lambda a: torch.tensor(a, dtype=torch.float32)
    lr_f, b1_f, b2_f = float(np.float32(lr)), float(np.float32(b1)), float(np.float32(b2))
    inv_sqrt_bc2 = f(1.0 / np.sqrt(1.0 - b2_f ** step))
    step_size = f(lr_f / (1.0 - b1_f ** step))
    one = f(1.0)
    gi = g * f(gs)
    pi = p * (one - f(lr) * f(wd))
    mi = f(b1) * m + (one - f(b1)) * gi
    vi = f(b2) * v + (one - f(b2)) * gi * gi
    denom = torch.sqrt(vi) * inv_sqrt_bc2 + f(eps)
    return pi - step_size * mi / denom, mi, vi


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000003])
def test_adamw_hyperparameters(dev, n):
    """Every hyper-parameter off its default, grad_scale included; steps 1-3 and one numbered 10 000 (bias corrections near
    1); exactly-zero gradient entries; p, m AND v compared."""
    from clipfs import ops
    from oracle import clip_oracle as O
    hp = dict(lr=1e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.1)
    gs = 0.25
    p64 = (_rand(n, seed=1) * 0.05).float().double()
    g0 = (_rand(n, seed=2) * 1e-2).float()
    g0[1::3] = 0.0
    m64, v64 = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    p32, m32, v32 = p64.float(), m64.float(), v64.float()
    pd, md, vd = p32.to(dev), m32.to(dev), v32.to(dev)
    for step in (1, 2, 3, 10000):
        gstep = g0 * float(min(step, 4))
        if step == 2:
            gstep = gstep.roll(1)  # other entries are zero in this step
        p64, m64, v64 = O.jt_adamw_step(p64, gstep.double() * gs, m64, v64, step, **hp)
        p32, m32, v32 = _adamw_f32(p32, gstep, m32, v32, step, hp["lr"], *hp["betas"], hp["eps"], hp["weight_decay"], gs)
        ops.adamw(pd, gstep.to(dev), md, vd, step, grad_scale=gs, **hp)
    # no direct tolerance existed for these hyper-parameters: 4 x the float32 restatement's error against fp64 after the
    # four steps.  Measured on the CPU: n = 1 000 003: p 4.9e-8, m 2.1e-9, v 5.0e-11 -> bounds 2.0e-7, 8.3e-9, 2.0e-10;
    # n = 255 - 257: p 2.0e-8, m 7.5e-10, v 1.8e-11; n = 1: p 5.8e-10, m 1.4e-10, v 1.9e-13 (|p| <= 0.24, |m| <= 1.7e-2,
    # |v| <= 1.8e-4)
    for name, got, r32, want in (("p", pd, p32, p64), ("m", md, m32, m64), ("v", vd, v32, v64)):
        _close(got, want, 4 * _err(r32, want), f"adamw {name}")


# ------------------------------------------------------------------ C. token kernels
def test_gather_eot_second_lane_stride(dev):
    """seq = 77: positions 64 ... 76 are a lane's second element; the first of two copies of the largest id wins."""
    from clipfs import ops
    n, seq, width = 6, 77, 72
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(1, 1000, (n, seq), generator=g, dtype=torch.int64)
    for row, places in enumerate([(3, 70), (66, 70), (76,), (0, 64), (64, 65), (12, 76)]):
        ids[row, list(places)] = 49407
    x = torch.randn(n * seq, width, generator=g).to(dev)
    rows, idx = ops.gather_eot(x, ids.to(dev))
    want = ids.argmax(dim=-1)
    assert want.tolist() == [3, 66, 76, 0, 64, 12]
    assert torch.equal(idx.cpu().long(), want)
    assert _same_bits(rows, x.view(n, seq, width)[torch.arange(n), want.to(dev)].contiguous())


@pytest.mark.parametrize("n,seq,width,n_ctx", [(3, 5, 4, 2), (220, 77, 512, 4)])  # 2nd: n * seq * width / 4 > 8192 * 256
def test_text_embed_shapes(dev, n, seq, width, n_ctx):
    from clipfs import ops
    vocab = 300
    g = torch.Generator().manual_seed(n)
    ids = torch.randint(0, vocab, (n, seq), generator=g, dtype=torch.int64)
    table, pos, ctx = _rand(vocab, width, seed=1).float(), _rand(seq, width, seed=2).float(), _rand(n_ctx, width, seed=3).float()
    want = table[ids]
    # one fp32 addition per element: the float32 sum itself, bit for bit
    assert _same_bits(ops.text_embed(ids.to(dev), table.to(dev), pos.to(dev)).cpu(), (want + pos).view(n * seq, width))
    want[:, 1:1 + n_ctx] = ctx
    got = ops.text_embed(ids.to(dev), table.to(dev), pos.to(dev), ctx=ctx.to(dev))
    assert _same_bits(got.cpu(), (want + pos).view(n * seq, width))


def test_scatter_rows_past_grid_cap(dev):
    from clipfs import ops
    n, seq, width = 70, 77, 512  # n * seq * width > 8192 * 256 threads
    g = torch.Generator().manual_seed(2)
    dy = torch.randn(n, width, generator=g)
    idx = torch.randint(0, seq, (n,), generator=g, dtype=torch.int32)
    idx[-1] = seq - 1
    out = torch.full((n * seq, width), SENTINEL, device=dev)
    ops.scatter_rows(dy.to(dev), idx.to(dev), seq, out=out)
    want = torch.zeros(n, seq, width)
    want[torch.arange(n), idx.long()] = dy
    assert _same_bits(out.cpu(), want.view(n * seq, width))


def test_token_rows_grad_accumulates_at_an_offset(dev):
    from clipfs import ops
    n, seq, width, n_tok, first = 9, 77, 64, 4, 50
    dx = _rand(n * seq, width, seed=6).float()
    d0 = _rand(n_tok, width, seed=7).float()
    dctx = d0.clone().to(dev)
    ops.token_rows_grad(dx.to(dev), dctx, n, seq, first)
    want = d0.double() + dx.double().view(n, seq, width)[:, first:first + n_tok].sum(0)
    _close(dctx, want, 1e-5, "token rows grad")


@pytest.mark.parametrize("n_vpt", [0, 4])
def test_vit_fill_special_leaves_patch_rows(dev, n_vpt):
    from clipfs import ops
    B, P, width = 3, 4, 128
    L = 1 + P + n_vpt
    cls, pos = _rand(width, seed=1).float(), _rand(1 + P, width, seed=2).float()
    vpt = _rand(n_vpt, width, seed=3).float() if n_vpt else None
    x = torch.full((B * L, width), SENTINEL, device=dev)
    ops.vit_fill_special(x, cls.to(dev), pos.to(dev), vpt.to(dev) if n_vpt else None, B, L, P)
    x = x.view(B, L, width).cpu()
    assert _same_bits(x[:, 0].contiguous(), (cls + pos[0]).expand(B, -1).contiguous())
    assert (x[:, 1:1 + P] == SENTINEL).all(), "patch rows were written"
    if n_vpt:
        assert _same_bits(x[:, 1 + P:].contiguous(), vpt.expand(B, -1, -1).contiguous())
