"""clipfs_gemm_nt over every schedule class x epilogue x leading dimension, against ONE fp64 restatement of the epilogue.

The entry point is driven through ctypes so that the test owns every pointer: A, C, aux_out / aux_in and the residual sit
inside wider matrices (lda = K + 8, ldc = N + 12, ldres = N + 20, ldb = K + 4 for the exact kernels), every output is
followed by guard rows, the split-K workspace and the arrival counters by a tail.  Outputs, guards and tails are
pre-filled with one NaN bit pattern, the padding of every INPUT with NaN as well, so that

  * an element the kernel does not write, or computes from a padding element, fails the comparison (NaN);
  * an element the kernel writes where it must not fails the bit comparison of the guards.

Budgets are those of the existing tests of the same kernels (absolute, outputs are O(1)):
  exact fp32 1e-4 (test_gemm_epilogues), times max(1, |alpha|);  bf16 x 3 6e-5 (test_gemm_bf16x3);  f16 plane 2e-5
  against the fp64 product of the f16-rounded operands (test_gemm_f16_mode);  split vs unsplit 2e-5
  (test_gemm_splitk_matches_unsplit).
Every case prints its error before it asserts.  Worst seen on an MI355X over all cases of a precision:
  exact fp32 5.8e-6 (2600 x 1200 x 288, bias + LoRA r=17 + QuickGELU + residual);  bf16 x 3 4.0e-5 and f16 plane 3.2e-6
  (both 4100 x 3970 x 64, same epilogue);  split vs unsplit 7.6e-6 (995 x 1003 x 1056, bias);  planes with ldb != K 1.8e-6."""
import ctypes as C
from collections import OrderedDict

import pytest
import torch

from gemm_matrix_cases import (BK, PLANE_SHAPES, SCHEDULE_CLASSES, ceil_div, lora_seg_width, plane_big_tile)
from gemm_matrix_helpers import SENT, _embed, _err, _nan_f32, _untouched, ref_gemm

pytestmark = pytest.mark.gpu

GUARD_ROWS = 3
WS_TAIL = 4096             # floats behind the workspace
CNT_TAIL = 64              # ints behind the counters
LORA_SCALE = 0.5
BUDGET = {"fp32": 1e-4, "bf16x3": 6e-5, "f16_plane": 2e-5}
SPLIT_VS_UNSPLIT = 2e-5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


# ------------------------------------------------------------------ epilogue variants
def _epi(name, **kw):
    d = dict(name=name, alpha=1.0, bias=False, residual=False, act=0, aux_out=True, lora_r=0)
    d.update(kw)
    return d


EPILOGUES = [
    _epi("plain"),
    _epi("bias", bias=True),
    _epi("alpha_bias", alpha=0.125, bias=True),
    _epi("bias_res", bias=True, residual=True),
    _epi("act1_aux", act=1),
    _epi("act1_noaux", act=1, aux_out=False),
    _epi("act2", act=2),
    _epi("act2_res", act=2, residual=True),
    _epi("act3_bias_res", act=3, bias=True, residual=True),
    _epi("bias_lora4_res", bias=True, lora_r=4, residual=True),
    _epi("lora3", lora_r=3),                                   # odd rank: the masked half K-step of the LoRA MFMAs
    _epi("alpha_lora4", alpha=0.5, lora_r=4),                  # alpha != 1: the per-element LoRA path
    _epi("bias_lora17_act1_res", bias=True, lora_r=17, act=1, residual=True),
]
EPI = {e["name"]: e for e in EPILOGUES}
LORA_RANKS = sorted({e["lora_r"] for e in EPILOGUES if e["lora_r"]})


# ------------------------------------------------------------------ inputs, once per shape
class Problem:
    """Seeded inputs of one (shape, layout), their device images and the fp64 products; shared by every variant."""

    def __init__(self, dev, M, N, K, *, pad, ldb_pad, patch=None):
        g = torch.Generator().manual_seed(1000003 * M + 1009 * N + K)
        rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
        self.M, self.N, self.K, self.dev, self.patch = M, N, K, dev, patch
        self.ldc, self.ldres = N + 12, N + 20
        self.ldb = K + 4 if ldb_pad else K
        self.b = rnd(N, K) * K ** -0.5
        if patch is None:
            self.a = rnd(M, K)
            self.lda = K + 8 if pad else K
            self.a_dev = _embed(self.a, M + GUARD_ROWS, self.lda, dev)
            self.rows = torch.arange(M)                      # output row of GEMM row m
            self.out_rows = M + GUARD_ROWS
            self.res = rnd(M, N)
            self.res_dev = _embed(self.res, M + GUARD_ROWS, self.ldres, dev)
        else:
            B, R, ps = patch
            G = R // ps
            P = G * G
            assert M == B * P and K == 3 * ps * ps
            img = rnd(B, 3, R, R)
            # row m = (b, py, px), column k = (c, ky, kx)
            self.a = img.reshape(B, 3, G, ps, G, ps).permute(0, 2, 4, 1, 3, 5).reshape(M, K).contiguous()
            self.lda = 0
            self.a_dev = _nan_f32(B + 1, 3, R, R, dev=dev)   # one NaN image behind the batch
            self.a_dev[:B] = img.to(dev)
            self.out_tokens = P + 2                          # class token, P patches, one more slot
            m = torch.arange(M)
            self.rows = (m // P) * self.out_tokens + 1 + m % P
            self.out_rows = (B + 1) * self.out_tokens + GUARD_ROWS  # the token buffer holds one more image
            pos = rnd(P + 1, N)                              # row 0 belongs to the class token: never read
            self.res = pos[1 + m % P]
            self.res_dev = _embed(pos[1:], self.out_tokens + GUARD_ROWS, self.ldres, dev, row_index=torch.arange(1, P + 1))
        self.b_dev = _embed(self.b, N + GUARD_ROWS, self.ldb, dev)
        self.bias = rnd(N)
        self.bias_dev = _embed(self.bias[None], 2, N, dev).reshape(-1)
        self.aux_in = rnd(M, N)
        assert (self.aux_in > 0).any() and (self.aux_in < 0).any()
        self.aux_in_dev = _embed(self.aux_in, self.out_rows, self.ldc, dev, row_index=self.rows)
        self.seg = lora_seg_width(N)
        self.lora = {}
        for r in LORA_RANKS:
            t, lb = rnd(M, 3 * r), rnd(N, r)
            self.lora[r] = (t, lb, _embed(t, M + GUARD_ROWS, 3 * r, dev), _embed(lb, N + GUARD_ROWS, r, dev))
        self.acc = {}      # reference kind -> fp64 product
        self.planes = {}   # b_format -> device planes of the contiguous B

    def product(self, kind):
        if kind not in self.acc:
            a, b = (self.a.half(), self.b.half()) if kind == "f16_rounded" else (self.a, self.b)
            self.acc[kind] = a.double() @ b.double().t()
        return self.acc[kind]

    def b_planes(self, lib, b_format):
        if b_format not in self.planes:
            src = self.b.to(self.dev).contiguous()
            n = src.numel()
            if b_format == 1:
                pl = torch.empty(2 * n, dtype=torch.int16, device=self.dev)
                rc = lib.clipfs_split_bf16(src.data_ptr(), pl.data_ptr(), n, None)
            else:
                pl = torch.empty(n, dtype=torch.float16, device=self.dev)
                rc = lib.clipfs_convert_f16(src.data_ptr(), pl.data_ptr(), n, None)
            assert rc == 0, lib.clipfs_last_error()
            torch.cuda.synchronize()
            self.planes[b_format] = (pl, src)
        return self.planes[b_format]


_PROBLEMS = OrderedDict()


def problem(dev, M, N, K, *, pad=True, ldb_pad=True, patch=None):
    key = (M, N, K, pad, ldb_pad, patch)
    if key not in _PROBLEMS:
        while len(_PROBLEMS) >= 2:  # cases arrive grouped by shape: keep the memory of two
            _PROBLEMS.popitem(last=False)
        _PROBLEMS[key] = Problem(dev, M, N, K, pad=pad, ldb_pad=ldb_pad, patch=patch)
    return _PROBLEMS[key]


# ------------------------------------------------------------------ the one driver
def run_gemm(dev, shape, epilogue, *, precision="fp32", split=True, pad=True, patch=None, ldb_pad=None, expect_rc=0,
             expect_plan=None):
    """One clipfs_gemm_nt call on padded, guarded buffers.  Asserts first that clipfs_gemm_plan answers `expect_plan`
    (fields of the plan) for the very arguments of the call, then that the guards of C / aux_out, the workspace tail
    and the counters are as the call found them; returns (C [M,N], aux_out [M,N] or None, bits of both whole buffers)."""
    from clipfs import _lib
    lib = _lib.load()
    M, N, K = shape
    e = epilogue
    planes = precision != "fp32"
    if ldb_pad is None:
        ldb_pad = not planes  # the 16-bit-plane kernels require ldb == K
    p = problem(dev, M, N, K, pad=pad, ldb_pad=ldb_pad, patch=patch)
    c_buf = _nan_f32(p.out_rows, p.ldc, dev=dev)
    aux_buf = _nan_f32(p.out_rows, p.ldc, dev=dev)
    nws = lib.clipfs_gemm_workspace_floats(M, N, K) if split else 0
    ncnt = lib.clipfs_gemm_counter_ints(M, N, K) if split else 0
    ws = _nan_f32(nws + WS_TAIL, dev=dev)
    cnt = torch.zeros(ncnt + CNT_TAIL, dtype=torch.int32, device=dev)

    g = _lib.new_gemm_args()
    g.A, g.C = p.a_dev.data_ptr(), c_buf.data_ptr()
    g.M, g.N, g.K = M, N, K
    g.lda, g.ldb, g.ldc = p.lda, p.ldb, p.ldc
    g.alpha = e["alpha"]
    g.act = e["act"]
    if e["bias"]:
        g.bias = p.bias_dev.data_ptr()
    if e["residual"]:
        g.residual, g.ldres = p.res_dev.data_ptr(), p.ldres
    if e["aux_out"]:
        g.aux_out = aux_buf.data_ptr()  # ignored unless act == 1: then the whole buffer keeps the sentinel
    if e["act"] == 2:
        g.aux_in = p.aux_in_dev.data_ptr()
    if e["lora_r"]:
        _, _, t_dev, lb_dev = p.lora[e["lora_r"]]
        g.lora_t, g.lora_b = t_dev.data_ptr(), lb_dev.data_ptr()
        g.lora_r, g.lora_nseg, g.lora_seg_width, g.lora_scale = e["lora_r"], 3, p.seg, LORA_SCALE
    if patch is not None:
        g.a_mode = 1
        g.img_res, g.patch, g.out_tokens = patch[1], patch[2], p.out_tokens
    keep = None
    if planes:
        pl, src = keep = p.b_planes(lib, 1 if precision == "bf16x3" else 2)
        g.B_planes, g.b_format = pl.data_ptr(), (1 if precision == "bf16x3" else 2)
        g.B = p.b_dev.data_ptr() if ldb_pad else src.data_ptr()
    else:
        g.B = p.b_dev.data_ptr()
    if split:
        g.workspace, g.workspace_floats = ws.data_ptr(), nws
        g.counters, g.counters_ints = cnt.data_ptr(), ncnt
    for ptr in (g.A, g.B, g.C, g.workspace, g.B_planes):
        assert not ptr or ptr % 16 == 0
    assert g.lda % 4 == 0 and g.ldb % 4 == 0
    if expect_plan:
        plan = _lib.gemm_plan(g)
        assert {k: plan[k] for k in expect_plan} == expect_plan, plan

    rc = lib.clipfs_gemm_nt(C.byref(g), torch.cuda.current_stream().cuda_stream)
    assert rc == expect_rc, (rc, lib.clipfs_last_error())
    torch.cuda.synchronize()
    del keep
    if rc != 0:
        assert _untouched(c_buf) and _untouched(aux_buf) and _untouched(ws) and not cnt.any().item()
        return None

    rows = p.rows.to(dev)
    writes_aux = e["act"] == 1 and e["aux_out"]
    for what, buf, written in (("C", c_buf, True), ("aux_out", aux_buf, writes_aux)):
        bits = buf.view(torch.int32).clone()
        if written:
            bits[:, :N][rows] = SENT
        bad = (bits != SENT).nonzero()
        assert bad.numel() == 0, f"{what}: {bad.shape[0]} elements outside [M, N] written, first (row, col) {bad[0].tolist()}"
    assert _untouched(ws[nws:]), "the workspace was written past clipfs_gemm_workspace_floats"
    assert not cnt.any().item(), f"arrival counters not zero on return: {cnt.nonzero().flatten()[:8].tolist()}"
    out = c_buf[:, :N][rows].cpu()
    aux = aux_buf[:, :N][rows].cpu() if writes_aux else None
    return out, aux, (c_buf.view(torch.int32), aux_buf.view(torch.int32))


def check_case(dev, shape, epi_name, *, kernel, tile_rows=64, precision="fp32", patch=None, ldb_pad=None, splits=1, budget_of=None,
               plan_splits=None):
    """(a) - (f) of the module docstring's contract for one case; `kernel`, `tile_rows` and `splits` (`plan_splits` where
    the case does not compare against the unsplit kernel) are what the plan of every launch must name."""
    e = EPI[epi_name]
    M, N, K = shape
    plan_splits = plan_splits or splits
    want_plan = dict(kernel=kernel, tile_rows=tile_rows, splits=plan_splits, want_splits=plan_splits)
    out, aux, bits = run_gemm(dev, shape, e, precision=precision, patch=patch, ldb_pad=ldb_pad, expect_plan=want_plan)
    p = problem(dev, M, N, K, pad=True, ldb_pad=(precision == "fp32") if ldb_pad is None else ldb_pad, patch=patch)
    budget_of = budget_of or precision
    kind = "f16_rounded" if budget_of == "f16_plane" else "exact"
    lora = None
    if e["lora_r"]:
        t, lb = p.lora[e["lora_r"]][:2]
        lora = (t.double(), lb.double(), p.seg, LORA_SCALE)
    want, pre = ref_gemm(None, None, acc=p.product(kind), alpha=e["alpha"], bias=p.bias.double() if e["bias"] else None,
                         lora=lora, act=e["act"], aux_in=p.aux_in.double() if e["act"] == 2 else None,
                         residual=p.res.double() if e["residual"] else None)
    budget = BUDGET[budget_of] * max(1.0, abs(e["alpha"]))
    # (a) the result and the saved pre-activation
    err = _err(out, want)
    errs = [err]
    if aux is not None:
        errs.append(_err(aux, pre))
    tag = budget_of if budget_of == precision else f"{precision} planes with ldb != K -> {budget_of}"
    print(f"[gemm-matrix] {tag} {shape} {epi_name}: err {max(errs):.3e} (budget {budget:.1e})")
    assert err <= budget, f"C: max abs err {err:.3e} > {budget:.1e}"
    if aux is not None:
        assert errs[1] <= budget, f"aux_out: max abs err {errs[1]:.3e} > {budget:.1e}"
    if e["act"] == 3:
        assert (out == 0).any() and (out > 0).any() and not (out < 0).any(), "ReLU case must clip some and keep some"
    # (b) - (d) were asserted by run_gemm;  (e) a second call into fresh buffers gives the same bits
    out2, aux2, bits2 = run_gemm(dev, shape, e, precision=precision, patch=patch, ldb_pad=ldb_pad, expect_plan=want_plan)
    assert torch.equal(bits[0], bits2[0]) and torch.equal(bits[1], bits2[1]), "not bitwise reproducible"
    # (f) split-K against the unsplit kernel on the same inputs
    if splits > 1:
        out_u, aux_u, _ = run_gemm(dev, shape, e, precision=precision, patch=patch, ldb_pad=ldb_pad, split=False,
                                   expect_plan=dict(want_plan, splits=1))
        d = _err(out, out_u.double())
        if aux is not None:
            d = max(d, _err(aux, aux_u.double()))
        print(f"[gemm-matrix] split vs unsplit {shape} {epi_name}: {d:.3e} (budget {SPLIT_VS_UNSPLIT:.1e})")
        assert d <= SPLIT_VS_UNSPLIT, f"split vs unsplit {d:.3e} > {SPLIT_VS_UNSPLIT:.1e}"


# ------------------------------------------------------------------ exact fp32: every schedule class x every epilogue
FP32_CASES = [(c, e["name"]) for c in SCHEDULE_CLASSES for e in EPILOGUES]


@pytest.mark.parametrize("c,epi", FP32_CASES, ids=[f"{c.name}-{e}" for c, e in FP32_CASES])
def test_fp32_schedule_class(dev, c, epi):
    from clipfs import _lib
    lib = _lib.load()
    # the class first: a retune of the heuristics must fail here, not silently run another kernel
    assert lib.clipfs_gemm_tile_rows(c.M, c.N) == c.tile_rows
    assert lib.clipfs_gemm_splits(c.M, c.N, c.K) == c.S
    assert ceil_div(c.K, BK) == c.k_steps and (c.k_steps % c.S != 0) == c.uneven
    if c.S > 1:
        assert c.K % BK == 0 and lib.clipfs_gemm_workspace_floats(c.M, c.N, c.K) > 0
        assert lib.clipfs_gemm_counter_ints(c.M, c.N, c.K) > 0
    # the generic kernel exists with 64-row tiles only and never splits, whatever the shape-only queries answer
    kernel, rows = ("generic", 64) if c.K % BK else ("nt32", 32) if c.tile_rows == 32 else ("nt64", 64)
    check_case(dev, (c.M, c.N, c.K), epi, kernel=kernel, tile_rows=rows, splits=c.S)


# ------------------------------------------------------------------ 16-bit-plane kernels
PLANE_EPILOGUES = [e["name"] for e in EPILOGUES if e["act"] != 3]  # the entry point refuses act 3 with planes
PLANE_CASES = [(pr, s, e) for s in PLANE_SHAPES for pr in ("bf16x3", "f16_plane") for e in PLANE_EPILOGUES]


@pytest.mark.parametrize("precision,s,epi", PLANE_CASES, ids=[f"{pr}-{s.name}-{e}" for pr, s, e in PLANE_CASES])
def test_plane_kernels(dev, precision, s, epi):
    assert plane_big_tile(s.M, s.N) == s.big_tile and s.K % BK == 0
    check_case(dev, (s.M, s.N, s.K), epi, precision=precision, kernel="planes128" if s.big_tile else "planes64",
               tile_rows=128 if s.big_tile else 64)


@pytest.mark.parametrize("precision", ["bf16x3", "f16_plane"])
def test_plane_kernels_refuse_relu(dev, precision):
    s = PLANE_SHAPES[0]
    assert run_gemm(dev, (s.M, s.N, s.K), EPI["act3_bias_res"], precision=precision, expect_rc=1) is None
    from clipfs import _lib
    assert b"act 3" in _lib.load().clipfs_last_error()


@pytest.mark.parametrize("precision", ["bf16x3", "f16_plane"])
def test_planes_with_padded_ldb_fall_back_to_exact(dev, precision):
    """B_planes with ldb != K: the dispatch takes the exact kernel on B itself, so the fp32 budget against the UNROUNDED
    fp64 product must hold (the f16 plane kernel would miss it by two orders of magnitude)."""
    s = PLANE_SHAPES[1]
    check_case(dev, (s.M, s.N, s.K), "bias_lora4_res", precision=precision, ldb_pad=True, budget_of="fp32",
               splits=1, kernel="nt32", tile_rows=32, plan_splits=2)


# ------------------------------------------------------------------ patch-embed A-mode
PATCH_CASES = [((2, 48, 16), 96), ((2, 28, 14), 200)]  # (images, resolution, patch), width
PATCH_EPILOGUES = ["plain", "bias_res", "act1_aux", "act2_res", "bias_lora4_res"]


@pytest.mark.parametrize("epi", PATCH_EPILOGUES)
@pytest.mark.parametrize("patch,width", PATCH_CASES, ids=["patch16", "patch14_ragged_n"])
def test_patch_embed_mode(dev, patch, width, epi):
    """a_mode 1 on the generic kernel: out_row(m) skips every image's class-token slot; those rows, the spare slot behind
    the patches, the rows of the image behind the batch and the guard rows keep the sentinel (run_gemm's guard check)."""
    B, R, ps = patch
    M, K = B * (R // ps) ** 2, 3 * ps * ps
    check_case(dev, (M, width, K), epi, patch=patch, kernel="generic")
