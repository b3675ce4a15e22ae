"""The large-M band of clipfs_gemm_nt (dense unsplit fp32 products of 4096 rows or more; csrc/gemm.hip, gemm_mixed_rows64):
a launch that deals whole rounds of the workgroup slots as 64-row tiles and the rows behind them as 32-row tiles.

Every shape is the smallest M at which the host query reports the path (searched here, not written down), plus ragged
ones (M % 64 != 0 and M % 32 != 0; 9 748 is the bench's live-row count; N % 128 != 0).  M_min is one row past the boundary
between the heights, so the boundary lies inside every matrix.

  * against CPU fp64 with the budget of the GEMM matrix tests (exact fp32: 1e-4 absolute, outputs are O(1)), for the three
    epilogues the tower uses in the band: bias + residual, QuickGELU with the saved pre-activation, QuickGELU gradient;
  * bit for bit against the same product on 2 048 of the rows (first rows; rows around the height boundary), a call that
    lands below the band: the band only changes tile shape and order, never an element's k order.
Outputs sit in NaN-filled wider buffers with guard rows: an element not written, or written outside [M, N], fails.
"""
import ctypes as C

import pytest
import torch

from gemm_matrix_cases import SCHEDULE_CLASSES, ceil_div
from gemm_matrix_helpers import SENT, _embed, _err, _nan_f32, ref_gemm

BUDGET = 1e-4          # exact fp32, as in test_gemm_matrix_gpu.py
GUARD_ROWS = 3
BAND_SEARCH = range(2601, 20000)   # above every SCHEDULE_CLASSES shape
EPILOGUES = {
    "bias_res": dict(bias=True, residual=True, act=0),
    "act1_aux": dict(bias=True, residual=False, act=1),
    "act2": dict(bias=False, residual=False, act=2),
}


def _lib():
    from clipfs import _lib
    return _lib.load()


def _ragged(M, pred=lambda M: True):
    """the first M' >= M + 37 with M' % 32 != 0 (so M' % 64 != 0 too) that `pred` accepts"""
    return next(m for m in range(M + 37, BAND_SEARCH.stop) if m % 32 and pred(m))


def _first(pred):
    return next(M for M in BAND_SEARCH if pred(M))


def _mixed_min(N, K):
    return _first(lambda M: _lib().clipfs_gemm_mixed_rows64(M, N, K) > 0)


# ------------------------------------------------------------------ host only
def test_band_queries_are_consistent():
    lib = _lib()
    for N, K in ((512, 512), (512, 2048), (512, 1536), (2048, 512), (1536, 512), (1000, 64), (768, 768), (3072, 768)):
        for M in (4096, 4097, _ragged(4096), 8192, 8193, 9748, 12800, 31031):
            nbn = ceil_div(N, 128)
            rows64 = lib.clipfs_gemm_mixed_rows64(M, N, K)
            if lib.clipfs_gemm_splits(M, N, K) > 1:  # few tiles: split as before, the band leaves it alone
                tiles = ceil_div(M, lib.clipfs_gemm_tile_rows(M, N)) * nbn
                assert rows64 == 0 and lib.clipfs_gemm_counter_ints(M, N, K) == tiles
                assert lib.clipfs_gemm_workspace_floats(M, N, K) == lib.clipfs_gemm_splits(M, N, K) * tiles * lib.clipfs_gemm_tile_rows(M, N) * 128
                continue
            # the band is unsplit: what is launched needs no scratch and no counters, and the queries ask for none
            assert lib.clipfs_gemm_workspace_floats(M, N, K) == 0 and lib.clipfs_gemm_counter_ints(M, N, K) == 0
            if rows64:
                assert lib.clipfs_gemm_tile_rows(M, N) == 32, "the rows behind the 64-row tiles are 32-row tiles"
                assert rows64 % 64 == 0 and 0 < rows64 <= M
                t64 = rows64 // 64 * nbn
                assert ceil_div(t64, 512) * 512 - nbn < t64, "the 64-row part is whole rounds of the 512 slots, less than one m-block short"
    # the image tower's shapes keep one height
    for N, K in ((768, 768), (2304, 768), (3072, 768), (768, 3072)):
        assert lib.clipfs_gemm_tile_rows(12800, N) == 64
        assert lib.clipfs_gemm_mixed_rows64(12800, N, K) == 0
    # the bench's N = 512 products mix: one round of 64-row tiles, the rest in 32-row tiles
    assert lib.clipfs_gemm_mixed_rows64(9748, 512, 512) == 8192


def test_schedule_classes_and_per_rank_shapes_lie_below_the_band():
    lib = _lib()
    for c in SCHEDULE_CLASSES:
        assert lib.clipfs_gemm_tile_rows(c.M, c.N) == c.tile_rows and lib.clipfs_gemm_splits(c.M, c.N, c.K) == c.S
        assert lib.clipfs_gemm_mixed_rows64(c.M, c.N, c.K) == 0
        if c.S == 1:
            assert lib.clipfs_gemm_workspace_floats(c.M, c.N, c.K) == 0 and lib.clipfs_gemm_counter_ints(c.M, c.N, c.K) == 0
    # 32 images x 50 tokens, up to 51 captions x 77 tokens, and the 2 048-row reference of the bitwise tests
    for M in (1600, 51 * 77, 2048):
        for N, K in ((512, 512), (512, 2048), (2048, 512), (1536, 512), (768, 768), (2304, 768), (3072, 768), (768, 3072)):
            assert lib.clipfs_gemm_mixed_rows64(M, N, K) == 0
    for bad in ((0, 512, 512), (9748, 0, 512), (9748, 512, 0)):
        assert lib.clipfs_gemm_mixed_rows64(*bad) == 0


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


_INPUTS = {}


def _inputs(M, N, K):
    """seeded CPU inputs and the fp64 product, computed once per shape and left unchanged"""
    key = (M, N, K)
    if key not in _INPUTS:
        if len(_INPUTS) >= 2:
            _INPUTS.pop(next(iter(_INPUTS)))
        g = torch.Generator().manual_seed(7 * M + 3 * N + K)
        rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
        a, b = rnd(M, K), rnd(N, K) * K ** -0.5
        _INPUTS[key] = dict(a=a, b=b, bias=rnd(N), res=rnd(M, N), aux_in=rnd(M, N), acc=a.double() @ b.double().t())
    return _INPUTS[key]


def _run(dev, x, rows, N, K, epi):
    """clipfs_gemm_nt on rows `rows` (a slice) of the inputs x, into NaN-filled padded buffers; returns (C, aux_out or None)"""
    from clipfs import _lib as L
    lib = L.load()
    e = EPILOGUES[epi]
    M = rows.stop - rows.start
    lda, ldc, ldres = K + 8, N + 12, N + 20
    a_dev = _embed(x["a"][rows], M + GUARD_ROWS, lda, dev)
    b_dev = _embed(x["b"], N + GUARD_ROWS, K + 4, dev)
    c_buf, aux_buf = _nan_f32(M + GUARD_ROWS, ldc, dev=dev), _nan_f32(M + GUARD_ROWS, ldc, dev=dev)
    keep = [a_dev, b_dev]
    g = L.new_gemm_args()
    g.A, g.B, g.C = a_dev.data_ptr(), b_dev.data_ptr(), c_buf.data_ptr()
    g.M, g.N, g.K = M, N, K
    g.lda, g.ldb, g.ldc = lda, K + 4, ldc
    g.alpha, g.act = 1.0, e["act"]
    if e["bias"]:
        keep.append(x["bias"].to(dev))
        g.bias = keep[-1].data_ptr()
    if e["residual"]:
        keep.append(_embed(x["res"][rows], M + GUARD_ROWS, ldres, dev))
        g.residual, g.ldres = keep[-1].data_ptr(), ldres
    if e["act"] == 1:
        g.aux_out = aux_buf.data_ptr()
    if e["act"] == 2:
        keep.append(_embed(x["aux_in"][rows], M + GUARD_ROWS, ldc, dev))
        g.aux_in = keep[-1].data_ptr()
    rc = lib.clipfs_gemm_nt(C.byref(g), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.clipfs_last_error()
    torch.cuda.synchronize()
    for what, buf, written in (("C", c_buf, True), ("aux_out", aux_buf, e["act"] == 1)):
        bits = buf.view(torch.int32).clone()
        if written:
            bits[:M, :N] = SENT
        bad = (bits != SENT).nonzero()
        assert bad.numel() == 0, f"{what}: {bad.shape[0]} elements outside [M, N] written, first (row, col) {bad[0].tolist()}"
    return c_buf[:M, :N].cpu(), (aux_buf[:M, :N].cpu() if e["act"] == 1 else None)


def _check(dev, M, N, K, epi, slices):
    """the band product against fp64, then bit for bit against each row slice run as a product of its own below the band"""
    lib = _lib()
    x = _inputs(M, N, K)
    e = EPILOGUES[epi]
    out, aux = _run(dev, x, slice(0, M), N, K, epi)
    want, pre = ref_gemm(None, None, acc=x["acc"], bias=x["bias"].double() if e["bias"] else None, act=e["act"],
                         aux_in=x["aux_in"].double() if e["act"] == 2 else None,
                         residual=x["res"].double() if e["residual"] else None)
    errs = [_err(out, want)] + ([_err(aux, pre)] if aux is not None else [])
    print(f"[gemm-band] {(M, N, K)} {epi}: err {max(errs):.3e} (budget {BUDGET:.1e})")
    assert max(errs) <= BUDGET
    for s in slices:
        n = s.stop - s.start
        assert 0 <= s.start and s.stop <= M and lib.clipfs_gemm_mixed_rows64(n, N, K) == 0
        assert n < BAND_SEARCH.start, "the slice must land in an unchanged schedule class"
        out_s, aux_s = _run(dev, x, s, N, K, epi)
        assert torch.equal(out[s].view(torch.int32), out_s.view(torch.int32)), f"rows {s}: C differs from the product below the band"
        if aux is not None:
            assert torch.equal(aux[s].view(torch.int32), aux_s.view(torch.int32)), f"rows {s}: aux_out differs"


MIXED_SHAPES = [("min_m", 512, 64, None), ("bench_rows", 512, 96, 9748), ("ragged_n", 1000, 64, None), ("ragged_m_n", 1000, 64, "ragged")]


@pytest.mark.gpu
@pytest.mark.parametrize("epi", list(EPILOGUES))
@pytest.mark.parametrize("name,N,K,M", MIXED_SHAPES, ids=[s[0] for s in MIXED_SHAPES])
def test_mixed_heights(dev, name, N, K, M, epi):
    lib = _lib()
    m_min = _mixed_min(N, K)
    M = m_min if M is None else _ragged(m_min, lambda m: lib.clipfs_gemm_mixed_rows64(m, N, K) > 0) if M == "ragged" else M
    rows64 = lib.clipfs_gemm_mixed_rows64(M, N, K)
    assert 0 < rows64 < M, "the boundary between the heights must fall inside the matrix"
    assert lib.clipfs_gemm_mixed_rows64(m_min - 1, N, K) == 0
    if name in ("bench_rows", "ragged_m_n"):
        assert M % 64 and M % 32 and (M - rows64) % 32
    lo = rows64 - 1024
    _check(dev, M, N, K, epi, [slice(0, 2048), slice(lo, min(M, lo + 2048))])
