"""The row-softmax kernels behind the losses, and LayerNorm, at the range the product runs at: logits of standard
deviation 30, rows shifted by +-300, one class 120 above the rest (every other probability underflows in fp32), logit
scales of 100 and 1000 on unit features, LayerNorm rows offset by +-1000 or with one outlier channel of 300.  The same
question as test_attention_range_gpu.py: a softmax without its row maximum, a log of an underflowed probability or a
one-pass variance passes every test on unit-range inputs.

The fp64 references are the suite's own (oracle.clip_oracle, tpt_ref.py, contrastive_ref.py); the yardstick is the same
reference evaluated in fp32 and the acceptance is budget(floor, yard_err, want) of range_cases.py with each kernel's
existing tolerance as the floor.  Class counts 5, 64, 65, 403 (the 64-lane stride edges), 1 and 7 rows.

Measured on an MI355X, worst max abs error over the shapes of a kernel and regime / its budget at that case (the cap of
budget() never triggered):
  cross_entropy, _scaled   peaked     loss_rows 2.6e-06 / 2.1e-05, loss_sum 3.9e-05 / 7.0e-05, dlogits 4.9e-08 / 1.0e-06
                           shifted    loss_rows 4.8e-07 / 1.0e-05, loss_sum 2.6e-06 / 7.0e-05, dlogits 2.9e-08 / 1.0e-06
                           confident  loss_rows 1.4e-06 / 1.1e-05, loss_sum 1.4e-06 / 1.1e-05, dlogits 6.4e-09 / 1.0e-06
                           dlogits x 4096: 2.0e-04, 1.2e-04, 2.6e-05 / 4.1e-03; the record's scale and grad_scale give
                           the same figures
  kl_logits (x | t)        peaked | peaked 1.0e-05 / 2.3e-04, shifted | peaked 1.3e-06 / 1.0e-05,
                           peaked | shifted 2.2e-05 / 1.7e-04, shifted | shifted 2.9e-07 / 2.0e-06,
                           confident | peaked 1.9e-05 / 2.4e-04, peaked | confident 1.4e-05 / 2.6e-04,
                           confident | confident 3.6e-06 / 2.4e-04, shifted | confident 5.3e-07 / 1.5e-05;
                           dx at most 1.3e-07 / 2.0e-06
  logit_normalize          shifted 2.5e-05 / 1.0e-04, peaked 3.6e-07 / 1.0e-04
  logit_normalize_bwd      shifted 6.8e-10 / 3.5e-09 (7 x 5; 1.9e-07 / 3.3e-06 at 1 x 64), peaked 9.2e-09 / 5.4e-08
  layernorm_fwd, _fwd_f16  offset 6.2e-05 / 5.8e-04, outlier 3.4e-06 / 2.0e-05
  layernorm_fwd_lora (t)   offset 9.5e-05 / 8.9e-04, outlier 7.5e-07 / 2.0e-05
  layernorm_bwd, _bwd_rows offset 2.8e-05 / 1.9e-04, outlier 1.8e-07 / 5.0e-05
  tpt_objective            s100: entropy 2.2e-05 / 2.0e-04, loss 2.1e-06 / 3.7e-05, dtext 1.7e-05 / 4.3e-04
                           s1000-offset: entropy 9.2e-05 / 1.9e-04, loss 2.4e-05 / 6.8e-05, dtext 3.1e-03 / 9.4e-03
                           s1000-saturated: entropy 9.2e-05 / 1.3e-04, loss 6.8e-08 / 3.7e-05
  contrastive_objective    s 100: loss 2.5e-07 / 3.5e-06, loss_rows 5.8e-06 / 7.3e-05, dq 2.2e-06 / 1.1e-04, dk 1.8e-06 / 1.0e-04
                           s 1000: loss 4.3e-06 / 3.5e-05, loss_rows 5.8e-05 / 5.6e-04, dq 1.2e-04 / 1.1e-03, dk 1.3e-04 / 1.1e-03
  mta                      mode 2.5e-06 / 2.0e-05, logits 1.2e-03 / 6.8e-03

Three kernels missed their budgets as they stood and were corrected with this suite:
  kl_logits              formed log p as x - (max + log sum): log sum rounded to an ulp of the maximum, every log p of the row
                         shifted by it (3.7e-05 / 6.4e-06 at shifted | shifted), and the fast exp / log under q (log q - log p)
                         with log-ratios of ~100 (1.2e-03 / 2.9e-04 at peaked | shifted, 7 x 403).  Now (x - max) - log sum,
                         precise exp / log.
  logit_normalize_bwd    centred one row of 300 + N(0, 1) by a mean whose sum had rounded at 64 x 300 (5.9e-06 / 3.3e-06 at
                         1 x 64).  Now every mean is taken of z - z[0].
  contrastive_objective  the statistics kernel and the gradient kernels summed the dot product in two orders, so the z behind
                         lse and the gradient's z differed by ~1e-7 s, uncancelled in exp(z - lse) of a row's dominant key
                         (dq 1.3e-03 / 1.1e-03 at 33 x 130 x 64, s 1000; a tenth of that at s 100).  Now one order."""
import functools

import pytest
import torch

import range_cases as R
from contrastive_ref import contrastive_inputs, contrastive_ref
from tpt_ref import tpt_inputs, tpt_ref

pytestmark = pytest.mark.gpu

CLASSES, ROWS = (5, 64, 65, 403), (1, 7)
SHAPES = [(r, c) for c in CLASSES for r in ROWS]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _check(kernel, case, what, got, want, floor, yard):
    """finite, and within budget(floor, |yard - want|, want); prints the figures first"""
    got = got.detach().cpu()
    assert torch.isfinite(got.float()).all(), f"{kernel} {case} {what}: not finite"
    err, yard_err = R.max_err(got, want), R.max_err(yard, want)
    tol = R.budget(floor, yard_err, want)
    print(f"RANGE|{kernel}|{case}|{what}|err {err:.3e}|budget {tol:.3e}|yardstick {yard_err:.3e}")
    assert err <= tol, f"{kernel} {case} {what}: max abs err {err:.3e} > {tol:.3e}"


def _leaf(t, dt):
    return t.detach().to(dt).clone().requires_grad_()


# ---- cross entropy ---------------------------------------------------------------------------------------------------------
def _ce_targets(z, kind):
    """the dominant class of each row, or its smallest one (underflowed in `peaked` and `confident`), alternating from
    `kind` on row 0"""
    top, low = z.argmax(1), z.argmin(1)
    first_top = torch.arange(z.shape[0]) % 2 == (0 if kind == "dominant" else 1)
    return torch.where(first_top, top, low)


@functools.lru_cache(maxsize=None)
def _ce_case(rows, classes, regime, kind):
    from oracle import clip_oracle as O
    z = R.logit_inputs(rows, classes, regime, 100 * classes + rows)
    tgt = _ce_targets(z, kind)

    def ref(dt):
        x = _leaf(z, dt)
        per_row = torch.stack([O.jt_cross_entropy(x[r:r + 1], tgt[r:r + 1]) for r in range(rows)])
        per_row.mean().backward()  # O.jt_cross_entropy of the whole batch
        return per_row.detach(), x.grad
    return z, tgt, ref(torch.float64), ref(torch.float32)


@pytest.mark.parametrize("regime", R.LOGIT_REGIMES)
@pytest.mark.parametrize("rows,classes", SHAPES)
def test_cross_entropy(dev, rows, classes, regime):
    """per-row loss, dlogits and the hit count of clipfs_cross_entropy (grad_scale 1 and 4096) and of
    clipfs_cross_entropy_scaled (a record holding 4096), targets on the dominant and on an underflowed class: a loss of
    ~120 (confident) or more (peaked), not inf.  Floors: 1e-5 on the loss, 1e-6 x the gradient's scale (test_kernels_gpu.py)."""
    from clipfs import _lib, ops
    lib = _lib.load()
    for kind in ("dominant", "underflowed"):
        z, tgt, (loss64, grad64), (loss32, grad32) = _ce_case(rows, classes, regime, kind)
        if regime != "shifted" and classes > 5 and (rows > 1 or kind == "underflowed"):
            assert loss64.max().item() > (100 if regime == "confident" else 50), "a target on an underflowed class"
        zd, td = z.float().to(dev), tgt.to(dev)
        hits = int((z.argmax(1) == tgt).sum())
        for gs, record in ((1.0, None), (4096.0, None), (1.0, 4096.0)):
            dl = torch.full((rows, classes), float("nan"), device=dev)
            loss_rows = torch.full((2 * rows,), float("nan"), device=dev)
            loss_sum = torch.full((1,), float("nan"), device=dev)
            correct = torch.full((1,), -1, device=dev, dtype=torch.int32)
            head = (zd.data_ptr(), td.data_ptr(), dl.data_ptr(), loss_rows.data_ptr(), loss_sum.data_ptr(), correct.data_ptr(),
                    rows, classes, gs)
            if record is None:
                _lib.check(lib.clipfs_cross_entropy(*head, _stream()), "cross_entropy")
            else:
                state = ops.new_scaler_state(record, dev)
                _lib.check(lib.clipfs_cross_entropy_scaled(*head, state.data_ptr(), _stream()), "cross_entropy_scaled")
            scale = gs * (record or 1.0)
            case = f"{rows}x{classes} {regime} {kind} x{scale:g}{' record' if record else ''}"
            name = "cross_entropy_scaled" if record else "cross_entropy"
            _check(name, case, "loss_rows", loss_rows[:rows], loss64, 1e-5, loss32)
            _check(name, case, "loss_sum", loss_sum, loss64.sum().reshape(1), 1e-5 * rows, loss32.sum().reshape(1))
            _check(name, case, "dlogits", dl, grad64 * scale, 1e-6 * scale, grad32 * scale)
            assert correct.item() == hits, (case, correct.item(), hits)


# ---- kl_logits -------------------------------------------------------------------------------------------------------------
KL_PAIRS = [("peaked", "peaked"), ("shifted", "peaked"), ("peaked", "shifted"), ("shifted", "shifted"), ("confident", "peaked"),
            ("peaked", "confident"), ("confident", "confident"), ("shifted", "confident")]


@functools.lru_cache(maxsize=None)
def _kl_case(rows, classes, rx, rt):
    from oracle import clip_oracle as O
    x = R.logit_inputs(rows, classes, rx, 7 * classes + rows)
    t = R.logit_inputs(rows, classes, rt, 11 * classes + rows, winner_shift=1)  # confident x confident: other winners

    def ref(dt):
        xl = _leaf(x, dt)
        kl = O.kl_div(O.jt_log_softmax(xl, 1), O.jt_log_softmax(t.to(dt), 1), reduction="none").sum(1)
        kl.sum().backward()
        return kl.detach(), xl.grad
    return x, t, ref(torch.float64), ref(torch.float32)


@pytest.mark.parametrize("rx,rt", KL_PAIRS, ids=[f"{a}-{b}" for a, b in KL_PAIRS])
@pytest.mark.parametrize("rows,classes", SHAPES)
def test_kl_logits(dev, rows, classes, rx, rt):
    """per-row KL(softmax(t) || softmax(x)) and dx = p - q.  Floors: test_stage2.py holds the mean to 2e-6 max(1, |ref|) and
    dx to 1e-8 at a gradient scale of 1 / numel, which is 2.3e-6 per unit scale at its smallest shape (7 x 33): 2e-6
    max(1, max |ref|) on a row and 2e-6 on dx at scale 1."""
    from clipfs import ops
    x, t, (kl64, dx64), (kl32, dx32) = _kl_case(rows, classes, rx, rt)
    if (rx, rt) == ("confident", "confident") and classes > 5:
        assert kl64.min().item() > 100, "the two winners differ"
    loss_rows, dx = ops.kl_logits(x.float().to(dev), t.float().to(dev), want_grad=True, grad_scale=1.0)
    case = f"{rows}x{classes} x {rx} t {rt}"
    _check("kl_logits", case, "loss_rows", loss_rows, kl64, 2e-6 * max(1.0, kl64.abs().max().item()), kl32)
    _check("kl_logits", case, "dx", dx, dx64, 2e-6, dx32)


# ---- logit_normalize -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["shifted", "peaked"])
@pytest.mark.parametrize("rows,classes", SHAPES)
def test_logit_normalize(dev, rows, classes, regime):
    """(z - row mean) / std over all elements.  One shifted row is 300 + N(0, 1): a one-pass variance loses it in
    E[z^2] ~ 9e4.  Floors: 1e-4 forward (test_kernels_gpu.py); the backward has none, its budget is the yardstick's alone
    (test_glue_kernels_gpu.py: 4 x there, 8 x by this suite's rule)."""
    from clipfs import ops
    from oracle import clip_oracle as O
    z = R.logit_inputs(rows, classes, regime, 13 * classes + rows)
    dzn = R.logit_inputs(rows, classes, "unit", 17 * classes + rows)

    def ref(dt):
        x = _leaf(z, dt)
        zn = O.logit_normalize(x)
        zn.backward(dzn.to(dt))
        return zn.detach(), x.grad
    (zn64, dz64), (zn32, dz32) = ref(torch.float64), ref(torch.float32)
    zd = z.float().to(dev)
    case = f"{rows}x{classes} {regime}"
    _check("logit_normalize", case, "out", ops.logit_normalize(zd), zn64, 1e-4, zn32)
    _check("logit_normalize_bwd", case, "dz", ops.logit_normalize_bwd(zd, dzn.float().to(dev)), dz64, 0.0, dz32)


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------
LN_SHAPES = [(r, w) for w in (64, 768, 1024) for r in (5, 37)]


@functools.lru_cache(maxsize=None)
def _ln_case(rows, width, kind):
    """x, gamma, beta, dy, dres, A (fp64 holding fp32 values) and the (y, dx, t) of the oracle's LayerNorm in fp64 and fp32.
      offset   unit data + 1000 on even rows, - 1000 on odd rows
      outlier  unit data, channel 3 r + 1 of row r is 300"""
    from oracle import clip_oracle as O
    g = torch.Generator().manual_seed(rows * 10000 + width)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    x = r(rows, width)
    if kind == "offset":
        x = x + torch.where(torch.arange(rows) % 2 == 0, 1000.0, -1000.0).double()[:, None]
    else:
        x[torch.arange(rows), (3 * torch.arange(rows) + 1) % width] = 300.0
    gamma, beta, dy, dres = 1 + 0.1 * r(width), r(width), r(rows, width), r(rows, width)
    A = r(3 * 4, width) * width ** -0.5
    x, gamma, beta, dy, dres, A = (t.float().double() for t in (x, gamma, beta, dy, dres, A))

    def ref(dt):
        xl = _leaf(x, dt)
        y = O.jt_layer_norm(xl, gamma.to(dt), beta.to(dt))
        y.backward(dy.to(dt))
        return y.detach(), xl.grad + dres.to(dt), y.detach() @ A.to(dt).t()
    return (x, gamma, beta, dy, dres, A), ref(torch.float64), ref(torch.float32)


@pytest.mark.parametrize("kind", ["offset", "outlier"])
@pytest.mark.parametrize("rows,width", LN_SHAPES)
def test_layernorm(dev, rows, width, kind):
    """layernorm_fwd, _fwd_f16, _fwd_lora, _bwd and _bwd_rows.  Floors: 2e-5 forward, 5e-5 backward, 2e-5 on the fused
    down-projection (test_kernels_gpu.py); the f16 copy is y rounded once; the fused and the row-mapped entry points give
    the bits of the plain ones."""
    from clipfs import _lib, ops
    lib = _lib.load()
    (x, gamma, beta, dy, dres, A), (y64, dx64, t64), (y32, dx32, t32) = _ln_case(rows, width, kind)
    D = lambda t: t.float().to(dev)  # noqa: E731
    xd, gd, bd, dyd, dresd, Ad = (D(t) for t in (x, gamma, beta, dy, dres, A))
    case = f"{rows}x{width} {kind}"
    y, mean, rstd = ops.layernorm_fwd(xd, gd, bd, save_stats=True)
    _check("layernorm_fwd", case, "y", y, y64, 2e-5, y32)
    # fp16 storage mode: the same y, and its f16 copy
    yf = torch.full((rows, width), float("nan"), device=dev)
    y16 = torch.full((rows, width), float("nan"), device=dev, dtype=torch.float16)
    m2, r2 = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
    _lib.check(lib.clipfs_layernorm_fwd_f16(xd.data_ptr(), width, gd.data_ptr(), bd.data_ptr(), yf.data_ptr(), y16.data_ptr(),
                                            m2.data_ptr(), r2.data_ptr(), rows, width, 1e-5, _stream()), "layernorm_fwd_f16")
    assert torch.equal(yf, y) and torch.equal(m2, mean) and torch.equal(r2, rstd) and torch.equal(y16, y.half())
    _check("layernorm_fwd_f16", case, "y", yf, y64, 2e-5, y32)
    # fused with the adapter down-projection (no dropout, all three segments)
    assert lib.clipfs_layernorm_fwd_lora_ok(width, 4, 3) == 1
    yl, t, m3, r3 = ops.layernorm_fwd_lora(xd, gd, bd, Ad, 4, 3)
    assert torch.equal(yl, y) and torch.equal(m3, mean) and torch.equal(r3, rstd)
    _check("layernorm_fwd_lora", case, "t", t, t64, 2e-5, t32)
    # backward, plain and through a row map
    dx = ops.layernorm_bwd(dyd, xd, gd, mean, rstd, dres=dresd)
    _check("layernorm_bwd", case, "dx", dx, dx64, 5e-5, dx32)
    perm = torch.randperm(rows, generator=torch.Generator().manual_seed(rows)).to(torch.int32)
    pl = perm.long()
    dxr = torch.full((rows, width), float("nan"), device=dev)
    dy_p, dres_p = dyd[pl.to(dev)].contiguous(), dresd[pl.to(dev)].contiguous()
    _lib.check(lib.clipfs_layernorm_bwd_rows(dy_p.data_ptr(), xd.data_ptr(), width, gd.data_ptr(), mean.data_ptr(),
                                             rstd.data_ptr(), perm.to(dev).data_ptr(), dres_p.data_ptr(), dxr.data_ptr(), width,
                                             rows, width, _stream()), "layernorm_bwd_rows")
    assert torch.equal(dxr, dx[pl.to(dev)])
    _check("layernorm_bwd_rows", case, "dx", dxr, dx64[pl], 5e-5, dx32[pl])


# ---- test-time prompt tuning objective ---------------------------------------------------------------------------------------
TPT_LOSS, TPT_ENT, TPT_DT = 3.7e-5, 1.3e-4, 1.2e-4  # test_tpt_gpu.py: loss, entropy, dtext as a share of its largest entry


def _tpt_inputs(V, C, d, spread):
    """tpt_inputs with every row pulled towards the common direction: cosines differ by `spread` x what they did, so a
    scale of 1000 at spread 0.3 gives logits of 975 .. 991, as far apart as at 100 but past exp's overflow"""
    F, T = tpt_inputs(V, C, d, seed=5)
    if spread == 1.0:
        return F, T
    m = torch.nn.functional.normalize(T.double().mean(0), dim=0)
    return tuple(torch.nn.functional.normalize(m + spread * (t.double() - m), dim=-1).float() for t in (F, T))


TPT_CASES = [(100.0, 1.0, True), (1000.0, 0.3, True), (1000.0, 1.0, False)]


@pytest.mark.parametrize("scale,spread,well_conditioned", TPT_CASES, ids=["s100", "s1000-offset", "s1000-saturated"])
@pytest.mark.parametrize("V,C,d,K", [(17, 10, 64, 4), (65, 403, 512, 6)])
def test_tpt_objective(dev, V, C, d, K, scale, spread, well_conditioned):
    """loss, entropy, selection and dtext on unit features at logit scales of 100 and 1000.
      s1000-offset     logits of 975 .. 991: every exp() overflows without the row maximum, the softmax is that of s100
      s1000-saturated  tpt_inputs as they are: logits of 740 .. 900, most views one-hot, entropies down to 1e-37 that tie
                       within rounding, pbar down to 1e-43 (it underflows in fp32: the kernel defines g = 0 there, and the
                       fp64 limit of every exposed output agrees, since g only ever meets a probability that underflowed
                       with it).  The gradient is what is left of terms of size s g / K ~ 1e4 that cancel to 5e-5
                       (1e-21 at 403 classes); tpt_ref.py calls it ill-conditioned, and the fp32 yardstick itself misses
                       it by 2.3e-3 of its largest entry at (17, 10, 64), past the cap of budget().  So there dtext is
                       held to being finite, and loss, entropy and selection to their budgets.
    Any selection that differs from the reference's only in views within the entropy budget of the K-th entropy is
    accepted, and loss and gradient are compared for the kernel's set (as test_tpt_gpu.py::test_objective_large_v does)."""
    from clipfs import ops
    F, T = _tpt_inputs(V, C, d, spread)
    assert (F.double().norm(dim=-1) - 1).abs().max() < 1e-6 and (T.double().norm(dim=-1) - 1).abs().max() < 1e-6
    _, _, H64, _ = tpt_ref(F, T, K, scale)
    _, _, H32, _ = tpt_ref(F, T, K, scale, dtype=torch.float32)
    loss, sel, dtext, ent = ops.tpt_objective(F.to(dev)[None], T.to(dev), K, scale, want_entropy=True)
    case = f"{V}x{C}x{d} K {K} s {scale:g} spread {spread:g}"
    _check("tpt_objective", case, "entropy", ent[0], H64, TPT_ENT, H32)
    got = sel[0].long().cpu()
    assert got.tolist() == sorted(set(got.tolist())) and got.numel() == K and 0 <= int(got[0]) and int(got[-1]) < V
    hk = torch.sort(H64).values[K - 1].item()
    tol = R.budget(TPT_ENT, R.max_err(H32, H64), H64)
    inside = torch.zeros(V, dtype=torch.bool)
    inside[got] = True
    assert (H64[inside] <= hk + tol).all() and (H64[~inside] >= hk - tol).all(), (got.tolist(), H64)
    loss64, dt64, _, _ = tpt_ref(F, T, K, scale, selected=got)
    loss32, dt32, _, _ = tpt_ref(F, T, K, scale, selected=got, dtype=torch.float32)
    _check("tpt_objective", case, "loss", loss[0].reshape(1), loss64.reshape(1), TPT_LOSS, loss32.reshape(1))
    assert torch.isfinite(dtext).all()
    if well_conditioned:
        _check("tpt_objective", case, "dtext", dtext[0], dt64, TPT_DT * dt64.abs().max().item(), dt32)


# ---- contrastive objective -------------------------------------------------------------------------------------------------
C_LOSS, C_ROWS, C_GRAD = 3.5e-6, 7.3e-5, 9.0e-5  # test_contrastive_gpu.py: loss_sum, loss_rows, dq / dk as a share
CONTRASTIVE = [(1, 1, 64, "paired"), (32, 32, 64, "paired"), (33, 130, 64, "groups")]


@functools.lru_cache(maxsize=None)
def _contrastive_case(Rq, N, d, kind, s):
    """the two smallest shapes of test_contrastive_gpu.py, and 130 keys: a second column chunk (the plan cuts at 128) whose
    two keys point away from the mean query and belong to no query's group, so it holds no positive and no maximum"""
    q, k, qg, kg = contrastive_inputs(Rq, N, d, kind)
    if N > 128:
        k = k.clone()
        k[128:] = -torch.nn.functional.normalize(q.double().mean(0), dim=0).float()
        kg[128:] = 10 ** 6
        z = q.double() @ k.double().t()
        assert (z[:, 128:].amax(1) < z[:, :128].amax(1) - 0.1).all() and not (qg[:, None] == kg[None, 128:]).any()
    w = 1.0 / Rq
    return q, k, qg, kg, contrastive_ref(q, k, qg, kg, s, w), contrastive_ref(q, k, qg, kg, s, w, dtype=torch.float32)


@pytest.mark.parametrize("s", [100.0, 1000.0])
@pytest.mark.parametrize("Rq,N,d,kind", CONTRASTIVE)
def test_contrastive_objective(dev, Rq, N, d, kind, s):
    from clipfs import _lib, ops
    assert _lib.contrastive_plan("stats", Rq, N, d)["chunks"] == (2 if N > 128 else 1)
    q, k, qg, kg, want, yard = _contrastive_case(Rq, N, d, kind, s)
    loss, rows, correct, dq, dk = ops.contrastive_objective(q.to(dev), k.to(dev), qg.to(dev), kg.to(dev), s, 1.0 / Rq)
    case = f"{Rq}x{N}x{d} {kind} s {s:g}"
    _check("contrastive_objective", case, "loss", loss, want["loss"].reshape(1), C_LOSS, yard["loss"].reshape(1))
    _check("contrastive_objective", case, "loss_rows", rows, want["loss_rows"], C_ROWS, yard["loss_rows"])
    for name, got in (("dq", dq), ("dk", dk)):
        top = want[name].abs().max().item()
        if top <= 1e-9 * s / Rq:  # one key: every term cancels, the reference is zero but for rounding
            assert got.abs().max().item() <= C_GRAD * s / Rq
            continue
        _check("contrastive_objective", case, name, got, want[name], C_GRAD * top, yard[name])
    if want["gap"] >= 1e-5 * s:
        assert correct.item() == want["correct"]


# ---- MTA -------------------------------------------------------------------------------------------------------------------
def test_mta_confident_affinities(dev):
    """the (17, 64, 10) shape of test_kernels_gpu.py::test_mta with the text rows scaled by 8: view logits of +-800, a
    softmax that is one-hot for most views, affinities of exactly 0 or 1.  Floors: 2e-5 on the mode, 1e-3 on the logits."""
    from clipfs import ops
    from oracle import clip_oracle as O
    V, d, Cn, n_img = 17, 64, 10, 3
    g = torch.Generator().manual_seed(4)
    base = torch.randn(n_img, 1, d, generator=g, dtype=torch.float64)
    feats = O.l2_normalize(base + 0.35 * torch.randn(n_img, V, d, generator=g, dtype=torch.float64)).float()
    text = (8.0 * O.l2_normalize(torch.randn(Cn, d, generator=g, dtype=torch.float64) + 0.5 * base[0])).float()
    mode, logits = ops.mta(feats.to(dev), text.to(dev))
    for i in range(n_img):
        sm = O.jt_softmax(feats[i].double() @ text.double().t() * 100, 1)
        assert (sm.amax(1) > 0.999).sum().item() >= V // 2, "most views are confident"
        want, yard = [[O.solve_mta(feats[i].to(dt), text.to(dt).t(), return_mode=m) for m in (True, False)]
                      for dt in (torch.float64, torch.float32)]
        _check("mta", f"image {i}", "mode", mode[i:i + 1], want[0], 2e-5, yard[0])
        _check("mta", f"image {i}", "logits", logits[i:i + 1], want[1], 1e-3, yard[1])
