"""Every attention kernel family on peaked, shifted and stairs scores (range_cases.py): scores of tens to hundreds, rows
whose exp() overflows fp32 without the row maximum and rows that underflow to l = 0 if the running maximum starts at 0, a
new maximum in every later key tile, whole tiles of probabilities that underflow.  The unit-normal inputs of every other
attention suite keep all scores within +-4, where a missing row maximum, a running maximum started at 0, a forgotten
online rescale and an lse in the wrong units are right to the last bit of the budgets (test_range_cases_cpu.py shows it).

Each case asserts the plan it ran (family, and nt / lmax where the family has instances), so coverage cannot move to
another kernel unnoticed, and checks
  * out, lse, dqkv finite (packed: the live rows; dead lse entries keep their NaN sentinel);
  * out, lse, dqkv against fp64 within budget(floor, yard_err, want) of range_cases.py: the family's existing budget, or
    8 x the error of a plain fp32 torch evaluation on the same inputs, capped at 1e-2 of the largest expected value;
      fp32 floors  out, lse 2e-5; dqkv 5e-5 max(1, max |grad|)
      f16 floors   out 2e-3 max(1, max |v|); lse 1e-3; dqkv 1e-2 max |grad|, yardstick with P rounded to f16
  * every out row inside the per-feature [min, max] of the v rows it sees (a convex combination: this catches a normaliser
    that disagrees with the weights even where both are near the reference), slack 1e-5 / 2e-3 of max |v|;
  * packed live rows bitwise the dense call's; the explicit long cut bitwise the default cut.

Measured on an MI355X, worst max abs error over the cases of a family / its budget at that case (the cap of budget() never
triggered; "hull" is how far an out row left the [min, max] of its v rows / the slack):
  family              regime    out                  lse                  dqkv                 hull
  mfma16 (nt 1,4,5,6) peaked    1.5e-05 / 1.0e-04    3.1e-05 / 1.3e-04    6.7e-05 / 5.4e-04    1.2e-07 / 3.3e-05
                      shifted   7.9e-05 / 6.1e-04    6.7e-05 / 4.2e-04    7.7e-04 / 7.2e-03    0 / 3.3e-05
                      stairs    1.4e-05 / 1.2e-04    1.1e-05 / 7.6e-05    1.1e-04 / 8.8e-04    0 / 3.3e-05
  mfma32              peaked    2.1e-05 / 1.3e-04    1.9e-05 / 1.5e-04    3.4e-05 / 3.8e-04    0 / 4.6e-05
                      shifted   5.9e-05 / 4.5e-04    7.4e-05 / 5.9e-04    5.5e-04 / 4.0e-03    0 / 4.6e-05
                      stairs    1.1e-04 / 8.1e-04    1.4e-05 / 9.1e-05    1.0e-04 / 7.6e-04    0 / 4.6e-05
  mfma_long (default  peaked    2.3e-05 / 1.4e-04    2.7e-05 / 1.8e-04    7.0e-05 / 6.7e-04    0 / 4.3e-05
  cut, and 64 / 1)    shifted   7.6e-05 / 7.0e-04    5.9e-05 / 5.8e-04    7.7e-04 / 7.3e-03    0 / 4.3e-05
                      stairs    1.2e-04 / 8.9e-04    6.0e-05 / 5.5e-04    1.1e-03 / 2.1e-02    0 / 4.3e-05
  stream, 1025        peaked    1.3e-05 / 2.2e-04    1.7e-05 / 2.2e-04    5.8e-05 / 8.3e-04    0 / 4.5e-05
                      shifted   4.9e-05 / 8.3e-04    3.5e-05 / 4.8e-04    9.9e-04 / 7.8e-03    0 / 4.5e-05
                      stairs    1.2e-04 / 1.7e-03    8.8e-05 / 9.7e-04    2.7e-04 / 8.5e-02    0 / 4.5e-05
  stream, misaligned  peaked    1.4e-05 / 1.5e-04    1.2e-05 / 1.3e-04    3.8e-05 / 6.4e-04    6.0e-08 / 3.9e-05
                      shifted   1.1e-04 / 6.4e-04    3.7e-05 / 4.1e-04    5.0e-04 / 6.7e-03    0 / 3.9e-05
                      stairs    3.0e-05 / 1.7e-04    1.9e-05 / 1.1e-04    7.9e-05 / 2.2e-03    0 / 3.9e-05
  recompute           peaked                                              2.1e-05 / 3.4e-04
  (lmax 64, 80, 96)   shifted                                             4.0e-04 / 7.0e-03
                      stairs                                              2.4e-05 / 7.1e-04
  mfma16 packed and   peaked    1.5e-05 / 1.4e-04    1.6e-05 / 2.5e-04    5.8e-05 / 7.8e-04    1.2e-07 / 4.0e-05
  pinned              shifted   7.2e-05 / 6.6e-04    7.1e-05 / 6.8e-04    6.4e-04 / 1.8e-02    0 / 4.0e-05
                      stairs    1.8e-05 / 1.6e-04    1.2e-05 / 1.6e-04    4.3e-05 / 5.0e-04    0 / 4.0e-05
  f16_short           peaked    4.4e-04 / 8.2e-03    1.0e-05 / 1.0e-03    6.4e-03 / 1.9e-01    2.4e-07 / 8.2e-03
                      shifted   3.9e-04 / 8.2e-03    4.6e-05 / 1.0e-03    5.6e-02 / 3.8e-01    0 / 8.9e-03
                      stairs    4.2e-04 / 8.2e-03    3.0e-05 / 1.0e-03    4.0e-02 / 2.8e-01    0 / 8.9e-03
  f16_long            peaked    3.1e-04 / 8.2e-03    1.3e-05 / 1.0e-03    3.0e-03 / 1.3e-01    0 / 8.6e-03
                      shifted   2.9e-04 / 8.6e-03    3.8e-05 / 1.0e-03    3.7e-02 / 4.4e-01    0 / 8.6e-03
                      stairs    3.6e-04 / 8.2e-03    4.1e-05 / 1.0e-03    6.9e-02 / 2.6e-01    0 / 8.6e-03
  f16 packed backward peaked    3.2e-04 / 7.9e-03    9.9e-06 / 1.0e-03    3.0e-03 / 1.6e-01    2.4e-07 / 7.9e-03
                      shifted   4.0e-04 / 7.9e-03    5.6e-05 / 1.0e-03    2.9e-02 / 3.3e-01    4.5e-05 / 7.9e-03
                      stairs    3.6e-04 / 7.9e-03    4.7e-06 / 1.0e-03    7.4e-03 / 9.9e-02    3.0e-05 / 7.9e-03
Every family passed as it stood; no attention kernel was changed.  The fp32 budgets are the widened ones (8 x the
yardstick) nearly everywhere, the f16 budgets are the floors except for out, where 8 x the P-rounding yardstick is larger."""
import pytest
import torch

import range_cases as R

pytestmark = pytest.mark.gpu

REGIMES = R.ATTENTION_REGIMES
F16 = torch.float16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _floors(qkv, want, f16):
    top = want[2].abs().max().item()
    if f16:
        vmax = qkv[:, 2 * qkv.shape[1] // 3:].abs().max().item()
        return 2e-3 * max(1.0, vmax), 1e-3, 1e-2 * top
    return 2e-5, 2e-5, 5e-5 * max(1.0, top)


class _Case:
    """one (shape, regime): the shared inputs and reference, and the checks against them"""

    def __init__(self, family, shape, regime, f16=False, lens=None):
        self.family, self.shape, self.regime, self.f16 = family, shape, regime, f16
        self.qkv, self.dout, self.want, self.yard = R.attention_case(*shape, regime, lens, F16 if f16 else None)
        self.floors = _floors(self.qkv, self.want, f16)
        self.live = None if lens is None else R.live_rows(shape[1], lens)

    def on(self, dev):
        return self.qkv.float().to(dev), self.dout.float().to(dev)

    def check(self, what, got, rows=None):
        """finite and within the budget; rows: the rows of the expected tensor that `got` holds"""
        i = ("out", "lse", "dqkv").index(what)
        want = self.want[i] if rows is None else self.want[i][rows]
        got = got.detach().cpu()
        assert torch.isfinite(got).all(), f"{self.family} {self.regime} {self.shape} {what}: not finite"
        err = R.max_err(got, want)
        tol = R.budget(self.floors[i], self.yard[i], self.want[i])
        print(f"RANGE|{self.family}|{self.regime}|{self.shape}|{what}|err {err:.3e}|budget {tol:.3e}|yardstick {self.yard[i]:.3e}")
        assert err <= tol, f"{self.family} {self.regime} {self.shape} {what}: max abs err {err:.3e} > {tol:.3e}"

    def check_convex(self, out, rows=None):
        lo, hi = R.visible_value_range(self.qkv, *self.shape)
        if rows is not None:
            lo, hi = lo[rows], hi[rows]
        slack = (2e-3 if self.f16 else 1e-5) * self.qkv[:, 2 * self.qkv.shape[1] // 3:].abs().max().item()
        o = out.detach().double().cpu()
        over = torch.maximum(lo - o, o - hi).max().item()
        print(f"RANGE|{self.family}|{self.regime}|{self.shape}|hull|err {max(over, 0.0):.3e}|budget {slack:.3e}|")
        assert over <= slack, f"{self.family} {self.regime} {self.shape}: out leaves the hull of its v rows by {over:.3e}"

    def check_all(self, out, lse, dqkv):
        self.check("out", out)
        self.check("lse", lse)
        self.check("dqkv", dqkv)
        self.check_convex(out)


def _plan_is(plan, family, **own):
    assert plan["family"] == family and all(plan[k] == v for k, v in own.items()), plan


# ---- exact fp32, default dispatch -------------------------------------------------------------------------------------------
DENSE = ([("mfma16", s, {"nt": nt}) for s, nt in R.MFMA16_SHAPES] + [("mfma32", s, {}) for s in R.MFMA32_SHAPES]
         + [("mfma_long", s, {}) for s in R.MFMA_LONG_SHAPES] + [("stream", R.STREAM_DEFAULT_SHAPE, {})])


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("family,shape,own", DENSE, ids=[f"{f}-{s[1]}" for f, s, _ in DENSE])
def test_fp32_default_dispatch(dev, family, shape, own, regime):
    from clipfs import _lib, ops
    for direction in ("fwd", "bwd"):
        _plan_is(_lib.attention_plan(direction, *shape), family, **own)
    c = _Case(family, shape, regime)
    qkv, dout = c.on(dev)
    out, lse = ops.attention_fwd(qkv, *shape, want_lse=True)
    dqkv = ops.attention_bwd(qkv, dout, *shape, out=out, lse=lse)
    c.check_all(out, lse, dqkv)


@pytest.mark.parametrize("regime", REGIMES)
def test_fp32_long_explicit_cut(dev, regime):
    """chunks of 64 tokens, runs of one tile: every wave rescales at every chunk; bit for bit the default cut"""
    from clipfs import _lib, ops
    shape = R.MFMA_LONG_SHAPES[1]
    _plan_is(_lib.attention_plan("fwd", *shape), "mfma_long")
    _plan_is(_lib.attention_plan("bwd", *shape), "mfma_long")
    c = _Case("mfma_long cut 64/1", shape, regime)
    qkv, dout = c.on(dev)
    out, lse = ops.attention_mfma_long_fwd(qkv, *shape, chunk_tokens=64, run_tiles=1)
    dqkv = ops.attention_mfma_long_bwd(qkv, dout, out, lse, *shape, chunk_tokens=64, run_tiles=1)
    c.check_all(out, lse, dqkv)
    out0, lse0 = ops.attention_fwd(qkv, *shape, want_lse=True)
    assert torch.equal(out, out0) and torch.equal(lse, lse0)
    assert torch.equal(dqkv, ops.attention_bwd(qkv, dout, *shape, out=out0, lse=lse0))


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("shape", R.STREAM_MISALIGNED_SHAPES, ids=lambda s: str(s[1]))
def test_fp32_streaming_through_misaligned_buffers(dev, shape, regime):
    """out and dqkv one float into a larger buffer (direct calls, NaN sentinels around the result)"""
    from clipfs import _lib
    lib = _lib.load()
    B, L, H, causal = shape
    for direction in ("fwd", "bwd"):
        _plan_is(_lib.attention_plan(direction, *shape, aligned=False), "stream")
    c = _Case("stream misaligned", shape, regime)
    qkv, dout = c.on(dev)
    n_out, n_qkv = dout.numel(), qkv.numel()
    nan = float("nan")
    obuf = torch.full((n_out + 9,), nan, device=dev)
    gbuf = torch.full((n_qkv + 9,), nan, device=dev)
    lse = torch.empty(B * H * L, device=dev)
    work = torch.empty_like(lse)
    assert all(t.data_ptr() % 16 == 0 for t in (qkv, dout, obuf, gbuf))
    _lib.check(lib.clipfs_attention_fwd(qkv.data_ptr(), obuf.data_ptr() + 4, lse.data_ptr(), B, L, H, int(causal), _stream()))
    _lib.check(lib.clipfs_attention_bwd(qkv.data_ptr(), dout.data_ptr(), obuf.data_ptr() + 4, lse.data_ptr(),
                                        gbuf.data_ptr() + 4, work.data_ptr(), B, L, H, int(causal), _stream()))
    torch.cuda.synchronize()
    for buf, n in ((obuf, n_out), (gbuf, n_qkv)):
        assert torch.isnan(buf[0]).item() and torch.isnan(buf[1 + n:]).all().item(), "a sentinel was overwritten"
    c.check_all(obuf[1:1 + n_out].reshape(dout.shape), lse, gbuf[1:1 + n_qkv].reshape(qkv.shape))


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("shape,lmax", R.RECOMPUTE_SHAPES, ids=[str(l) for _, l in R.RECOMPUTE_SHAPES])
def test_fp32_recomputing_backward(dev, shape, lmax, regime):
    """no out / lse from the forward: the kernel rebuilds the softmax itself"""
    from clipfs import _lib, ops
    _plan_is(_lib.attention_plan("bwd", *shape, stats=False), "recompute", lmax=lmax)
    c = _Case(f"recompute lmax {lmax}", shape, regime)
    qkv, dout = c.on(dev)
    c.check("dqkv", ops.attention_bwd(qkv, dout, *shape))


# ---- exact fp32, packed text rows ------------------------------------------------------------------------------------------
PACKED_SHAPE = (len(R.PACKED_LENS), R.PACKED_SEQ, R.PACKED_HEADS, True)


def _offsets(dev):
    off = torch.zeros(len(R.PACKED_LENS) + 1, dtype=torch.int32)
    off[1:] = torch.cumsum(torch.tensor(R.PACKED_LENS), 0).to(torch.int32)
    return off.to(dev), int(off[-1])


@pytest.mark.parametrize("regime", REGIMES)
def test_fp32_packed(dev, regime):
    """captions of 2, 17, 40 and 77 live tokens in one batch: the packed forward, the packed backward over full-layout
    tensors and the pinned backward over packed ones, each bitwise the dense call on the live rows"""
    from clipfs import _lib
    lib = _lib.load()
    B, L, H, _ = PACKED_SHAPE
    d = H * R.HD
    _plan_is(_lib.attention_plan("fwd", *PACKED_SHAPE), "mfma16", nt=5)
    _plan_is(_lib.attention_plan("bwd", *PACKED_SHAPE), "mfma16", nt=5)
    _plan_is(_lib.attention_plan("fwd_packed", *PACKED_SHAPE), "mfma16_packed", nt=5)
    _plan_is(_lib.attention_plan("bwd_packed", *PACKED_SHAPE), "mfma16_packed", nt=5)
    _plan_is(_lib.attention_plan("bwd_packed_io", *PACKED_SHAPE), "mfma16_pinned", nt=5)
    fwd, bwd, pin = (_Case(f, PACKED_SHAPE, regime, lens=R.PACKED_LENS)
                     for f in ("mfma16_packed fwd", "mfma16_packed bwd", "mfma16_pinned bwd"))
    live = fwd.live
    lse_live = live.view(B, 1, L).expand(B, H, L).reshape(-1)
    qf, dfull = fwd.on(dev)
    qp, dp = qf[live.to(dev)].contiguous(), dfull[live.to(dev)].contiguous()
    off, rows = _offsets(dev)
    nan = float("nan")
    out_f, lse_f = torch.zeros(B * L, d, device=dev), torch.zeros(B * H * L, device=dev)
    out_p, lse_p = torch.full((rows, d), nan, device=dev), torch.full((B * H * L,), nan, device=dev)
    dq_f, work = torch.zeros(B * L, 3 * d, device=dev), torch.empty(B * H * L, device=dev)
    dq_a, dq_b = torch.full((rows, 3 * d), nan, device=dev), torch.full((rows, 3 * d), nan, device=dev)
    st = _stream()
    _lib.check(lib.clipfs_attention_fwd(qf.data_ptr(), out_f.data_ptr(), lse_f.data_ptr(), B, L, H, 1, st))
    _lib.check(lib.clipfs_attention_fwd_packed(qp.data_ptr(), out_p.data_ptr(), lse_p.data_ptr(), off.data_ptr(), B, L, H, st))
    _lib.check(lib.clipfs_attention_bwd(qf.data_ptr(), dfull.data_ptr(), out_f.data_ptr(), lse_f.data_ptr(), dq_f.data_ptr(),
                                        work.data_ptr(), B, L, H, 1, st))
    _lib.check(lib.clipfs_attention_bwd_packed(qf.data_ptr(), dp.data_ptr(), out_f.data_ptr(), lse_f.data_ptr(),
                                               dq_a.data_ptr(), off.data_ptr(), B, L, H, st))
    _lib.check(lib.clipfs_attention_bwd_packed_io(qp.data_ptr(), dp.data_ptr(), out_p.data_ptr(), lse_p.data_ptr(),
                                                  dq_b.data_ptr(), off.data_ptr(), B, L, H, st))
    torch.cuda.synchronize()
    out_p, lse_p, dq_a, dq_b = out_p.cpu(), lse_p.cpu(), dq_a.cpu(), dq_b.cpu()
    assert torch.isnan(lse_p[~lse_live]).all(), "a dead lse entry was written"
    fwd.check("out", out_p, live)
    fwd.check("lse", lse_p[lse_live], lse_live)
    fwd.check_convex(out_p, live)
    bwd.check("dqkv", dq_a, live)
    pin.check("dqkv", dq_b, live)
    assert torch.equal(out_p, out_f.cpu()[live]) and torch.equal(lse_p[lse_live], lse_f.cpu()[lse_live])
    assert torch.equal(dq_a, dq_f.cpu()[live]) and torch.equal(dq_b, dq_a)


# ---- fp16 storage mode ------------------------------------------------------------------------------------------------------
F16_CASES = [("f16_short", s) for s in R.F16_SHORT_SHAPES] + [("f16_long", s) for s in R.F16_LONG_SHAPES]


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("qkv_f16", [False, True], ids=["qkv32", "qkv16"])
@pytest.mark.parametrize("family,shape", F16_CASES, ids=[f"{f}-{s[1]}" for f, s in F16_CASES])
def test_f16(dev, family, shape, qkv_f16, regime):
    from clipfs import _lib, ops
    for direction in ("fwd", "bwd"):
        _plan_is(_lib.attention_f16_plan(direction, *shape), family)
    c = _Case(family, shape, regime, f16=True)
    qkv, dout = c.on(dev)
    if qkv_f16:
        qkv = qkv.half()
    out, lse = ops.attention_f16_fwd(qkv, *shape)
    dqkv = ops.attention_f16_bwd(qkv, dout, out, lse, *shape)
    c.check_all(out, lse, dqkv)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("dout_f16", [False, True], ids=["dout32", "dout16"])
def test_f16_packed_backward(dev, dout_f16, regime):
    """the packed f16 backward on the dense forward's records: bitwise the dense backward on the live rows"""
    from clipfs import _lib, ops
    lib = _lib.load()
    B, L, H, _ = PACKED_SHAPE
    d = H * R.HD
    for direction in ("fwd", "bwd", "bwd_packed"):
        _plan_is(_lib.attention_f16_plan(direction, *PACKED_SHAPE), "f16_short")
    c = _Case("f16 packed bwd", PACKED_SHAPE, regime, f16=True, lens=R.PACKED_LENS)
    live = c.live
    qkv, dfull = c.on(dev)
    dp = dfull[live.to(dev)].contiguous()
    if dout_f16:
        dfull, dp = dfull.half(), dp.half()
    out, lse = ops.attention_f16_fwd(qkv, *PACKED_SHAPE)
    off, rows = _offsets(dev)
    nan = float("nan")
    dq_p = torch.full((rows, 3 * d), nan, device=dev)
    dq16_p = torch.full((rows, 3 * d), nan, device=dev, dtype=F16)
    work_p = torch.full((B * H * L,), nan, device=dev)
    dq_f = torch.zeros(B * L, 3 * d, device=dev)
    dq16_f = torch.zeros(B * L, 3 * d, device=dev, dtype=F16)
    work_f = torch.empty(B * H * L, device=dev)
    _lib.check(lib.clipfs_attention_f16_bwd_packed(qkv.data_ptr(), 0, dp.data_ptr(), int(dout_f16), out.data_ptr(), lse.data_ptr(),
                                                   dq_p.data_ptr(), dq16_p.data_ptr(), work_p.data_ptr(), off.data_ptr(), B, L,
                                                   H, _stream()))
    _lib.check(lib.clipfs_attention_f16_bwd(qkv.data_ptr(), 0, dfull.data_ptr(), int(dout_f16), out.data_ptr(), lse.data_ptr(),
                                            dq_f.data_ptr(), dq16_f.data_ptr(), work_f.data_ptr(), B, L, H, 1, _stream()))
    torch.cuda.synchronize()
    lse_live = live.view(B, 1, L).expand(B, H, L).reshape(-1)
    c.check("out", out.cpu()[live], live)
    c.check("lse", lse.cpu()[lse_live], lse_live)
    c.check_convex(out.cpu()[live], live)
    c.check("dqkv", dq_p, live)
    assert torch.isfinite(dq16_p.float()).all()
    assert torch.equal(dq_p.cpu(), dq_f.cpu()[live]) and torch.equal(dq16_p.cpu(), dq16_f.cpu()[live])
