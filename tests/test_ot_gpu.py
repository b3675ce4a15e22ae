"""OT matching on the GPU (csrc/ot_match.hip, ops.ot_*) against the fp64 rule of ot_ref.py on the cases of
ot_ref.CASES, each the smallest shape that reaches a distinct code path, at eps 0.05 / 0.1 / 1, 1 / 5 / 100 iterations,
uniform (NULL) and random marginals, spread and concentrated features, always with a z = -1 and a z = +1 cell.

The tolerance is not fixed in advance: per configuration tol = 16 x max(e32, 2^-24 max |ref|), e32 the error of the SAME
rule evaluated in fp32 on the CPU against its fp64 evaluation, for the logits, dP and dX separately.  Nothing from the
device enters the yardstick.  The factor 16 covers the different summation orders of the d-term dot products (which K
amplifies by 1 / eps) and of the M- and N-term sums.  Each parity test prints its worst measured / tol per output.

Measured on one MI355X, worst measured / tol over iterations, marginals and features (logits, dP, dX):

    case          eps 0.05             eps 0.1              eps 1
    plot          0.091 0.078 0.074    0.074 0.121 0.077    0.123 0.087 0.132
    two_rows_n1   0.134 0.134 0.125    0.151 0.118 0.073    0.103 0.159 0.127
    one_row       0.079 0.073 0.110    0.073 0.127 0.161    0.079 0.091 0.126
    four_rows     0.068 0.100 0.060    0.099 0.117 0.075    0.083 0.112 0.076
    n_cap         0.153 0.082 0.065    0.114 0.093 0.087    0.090 0.090 0.093
    straddle      0.064 0.082 0.103    0.082 0.080 0.134    0.060 0.091 0.130
    caps          0.103 0.118 0.083    0.132 0.188 0.108    0.062 0.213 0.088

The exact checks (run to run, poisoned outputs, NULL against explicit uniform marginals, an image or a class alone,
reversed classes, guard columns, autograd against ot_bwd) are bitwise."""
import pytest
import torch

import ot_ref as R
from poison import FILLS, poisoned, same_bits

pytestmark = pytest.mark.gpu
CASES = tuple(R.CASES)
EPSES = (0.05, 0.1, 1.0)
ITERS = (1, 5, 100)
SCALE = 100.0
_REF = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _dl(B, C, seed=7):
    return torch.randn(B, C, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).float()


def ref_case(case, feat, marg, eps, iters):
    """Inputs, dlogits and the fp64 / fp32 CPU evaluations, computed once, shared, never written."""
    key = (case, feat, marg, eps, iters)
    if key not in _REF:
        X, P, mu, nu = R.inputs(case, feat, marg)
        dl = _dl(X.shape[0], P.shape[0])
        r64 = R.grads(X, P, dl, mu, nu, eps, iters, SCALE, torch.float64)
        r32 = R.grads(X, P, dl, mu, nu, eps, iters, SCALE, torch.float32)
        _REF[key] = (X, P, mu, nu, dl, r64, r32)
    return _REF[key]


def _to(dev, *ts):
    return tuple(None if t is None else t.to(dev) for t in ts)


def _run(dev, X, P, mu, nu, dl, eps, iters):
    from clipfs import ops
    X, P, mu, nu, dl = _to(dev, X, P, mu, nu, dl)
    logits, u, v = ops.ot_logits(X, P, mu, nu, eps, iters, SCALE)
    dP, dX = ops.ot_bwd(X, P, u, v, dl, eps, SCALE, want_dx=True)
    return dict(logits=logits, u=u, v=v, dP=dP, dX=dX)


def _same(a, b):
    return all(same_bits(a[k], b[k]) for k in a)


# ------------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("eps", EPSES)
@pytest.mark.parametrize("case", CASES)
def test_parity_against_fp64(dev, case, eps):
    worst = dict(logits=0.0, dP=0.0, dX=0.0)
    fails = []
    for iters in ITERS:
        for marg in ("uniform", "random"):
            for feat in ("spread", "concentrated"):
                X, P, mu, nu, dl, r64, r32 = ref_case(case, feat, marg, eps, iters)
                out = _run(dev, X, P, mu, nu, dl, eps, iters)
                for k, (name, want, yard) in enumerate(zip(("logits", "dP", "dX"), r64, r32)):
                    got = out[name].double().cpu()
                    assert bool(torch.isfinite(got).all()), (case, eps, iters, marg, feat, name)
                    tol, e32 = R.tolerance(want, yard)
                    err = float((got - want).abs().max())
                    worst[name] = max(worst[name], err / tol)
                    if err > tol:
                        fails.append((iters, marg, feat, name, err, tol, e32))
    print(f"{case} eps {eps}: measured / tol  logits {worst['logits']:.3f}  dP {worst['dP']:.3f}  dX {worst['dX']:.3f}")
    assert not fails, fails


# ------------------------------------------------------------------------------------------------------- 2. exact
@pytest.mark.parametrize("case", CASES)
def test_bitwise_run_to_run_and_under_poison(dev, case):
    X, P, mu, nu, dl, _, _ = ref_case(case, "concentrated", "random", 0.1, 5)
    first = _run(dev, X, P, mu, nu, dl, 0.1, 5)
    assert _same(first, _run(dev, X, P, mu, nu, dl, 0.1, 5))
    for fill in FILLS:
        with poisoned(fill):
            assert _same(first, _run(dev, X, P, mu, nu, dl, 0.1, 5)), fill
    assert all(bool(torch.isfinite(t).all()) for t in first.values())


def test_null_marginals_are_the_uniform_ones(dev):
    """1 / M and 1 / N are the same fp32 number on both routes only for powers of two: M 64, N 4."""
    X, P, _, _ = R.inputs((2, 64, 3, 4, 32), "concentrated")
    dl = _dl(2, 3)
    mu, nu = torch.full((2, 64), 1.0 / 64), torch.full((3, 4), 1.0 / 4)
    assert _same(_run(dev, X, P, None, None, dl, 0.1, 20), _run(dev, X, P, mu, nu, dl, 0.1, 20))


@pytest.mark.parametrize("case", ("plot", "four_rows", "straddle"))
def test_an_image_or_a_class_alone_is_its_cell_of_the_full_call(dev, case):
    from clipfs import ops
    X, P, mu, nu, dl, _, _ = ref_case(case, "spread", "random", 0.1, 5)
    X, P, mu, nu, dl = _to(dev, X, P, mu, nu, dl)
    logits, u, v = ops.ot_logits(X, P, mu, nu, 0.1, 5, SCALE)
    dP, dX = ops.ot_bwd(X, P, u, v, dl, 0.1, SCALE, want_dx=True)
    for b in range(X.shape[0]):
        l1, u1, v1 = ops.ot_logits(X[b:b + 1].contiguous(), P, mu[b:b + 1].contiguous(), nu, 0.1, 5, SCALE)
        assert same_bits(l1, logits[b:b + 1]) and same_bits(u1, u[b:b + 1]) and same_bits(v1, v[b:b + 1]), b
        _, dX1 = ops.ot_bwd(X[b:b + 1].contiguous(), P, u1, v1, dl[b:b + 1].contiguous(), 0.1, SCALE, want_dx=True)
        assert same_bits(dX1, dX[b:b + 1]), b
    for c in range(P.shape[0]):
        l1, u1, v1 = ops.ot_logits(X, P[c:c + 1].contiguous(), mu, nu[c:c + 1].contiguous(), 0.1, 5, SCALE)
        assert same_bits(l1, logits[:, c:c + 1]) and same_bits(u1, u[:, c:c + 1]) and same_bits(v1, v[:, c:c + 1]), c
        dP1, _ = ops.ot_bwd(X, P[c:c + 1].contiguous(), u1, v1, dl[:, c:c + 1].contiguous(), 0.1, SCALE)
        assert same_bits(dP1, dP[c:c + 1]), c


@pytest.mark.parametrize("case", ("plot", "straddle"))
def test_reversed_classes_give_reversed_logits(dev, case):
    from clipfs import ops
    X, P, mu, nu, _, _, _ = ref_case(case, "spread", "random", 0.1, 5)
    X, P, mu, nu = _to(dev, X, P, mu, nu)
    logits, u, v = ops.ot_logits(X, P, mu, nu, 0.1, 5, SCALE)
    lr, ur, vr = ops.ot_logits(X, P.flip(0).contiguous(), mu, nu.flip(0).contiguous(), 0.1, 5, SCALE)
    assert same_bits(lr, logits.flip(1)) and same_bits(ur, u.flip(1)) and same_bits(vr, v.flip(1))


@pytest.mark.parametrize("fill", FILLS)
def test_guard_columns_keep_their_fill(dev, fill):
    from clipfs import ops
    X, P, mu, nu, dl, _, _ = ref_case("plot", "spread", "random", 0.1, 5)
    X, P, mu, nu, dl = _to(dev, X, P, mu, nu, dl)
    B, C = dl.shape
    logits, u, v = ops.ot_logits(X, P, mu, nu, 0.1, 5, SCALE)
    wide = torch.full((B, C + 3), fill, device=dev)
    ops.ot_logits(X, P, mu, nu, 0.1, 5, SCALE, out=wide[:, :C])
    assert same_bits(wide[:, :C], logits) and same_bits(wide[:, C:], torch.full((B, 3), fill, device=dev))
    # a padded dlogits reads its own columns only
    dwide = torch.full((B, C + 3), fill, device=dev)
    dwide[:, :C] = dl
    dP, dX = ops.ot_bwd(X, P, u, v, dl, 0.1, SCALE, want_dx=True)
    dP2, dX2 = ops.ot_bwd(X, P, u, v, dwide[:, :C], 0.1, SCALE, want_dx=True)
    assert same_bits(dP, dP2) and same_bits(dX, dX2)


@pytest.mark.parametrize("case", ("plot", "one_row"))
def test_accumulate_adds_to_the_outputs(dev, case):
    from clipfs import ops
    X, P, mu, nu, dl, _, _ = ref_case(case, "spread", "random", 0.1, 5)
    X, P, mu, nu, dl = _to(dev, X, P, mu, nu, dl)
    _, u, v = ops.ot_logits(X, P, mu, nu, 0.1, 5, SCALE)
    dP, dX = ops.ot_bwd(X, P, u, v, dl, 0.1, SCALE, want_dx=True)
    g = torch.Generator().manual_seed(3)
    p0, x0 = torch.randn(P.shape, generator=g).to(dev), torch.randn(X.shape, generator=g).to(dev)
    pa, xa = p0.clone(), x0.clone()
    ops.ot_bwd(X, P, u, v, dl, 0.1, SCALE, dp=pa, dx=xa, accumulate=True)
    for got, base, fresh in ((pa, p0, dP), (xa, x0, dX)):
        want = base.double() + fresh.double()
        assert bool(((got.double() - want).abs() <= 2.0 ** -23 * want.abs() + 1e-45).all())  # 1 ulp of the sum
    # without the flag the given outputs are overwritten
    ops.ot_bwd(X, P, u, v, dl, 0.1, SCALE, dp=pa, dx=xa)
    assert same_bits(pa, dP) and same_bits(xa, dX)


def test_autograd_is_ot_bwd(dev):
    from clipfs import ops
    X, P, mu, nu, dl, _, _ = ref_case("plot", "concentrated", "random", 0.1, 100)
    X, P, mu, nu, dl = _to(dev, X, P, mu, nu, dl)
    logits, u, v = ops.ot_logits(X, P, mu, nu, 0.1, 100, SCALE)
    dP, dX = ops.ot_bwd(X, P, u, v, dl, 0.1, SCALE, want_dx=True)
    Xg, Pg = X.clone().requires_grad_(True), P.clone().requires_grad_(True)
    out = ops.ot_match(Xg, Pg, mu, nu, eps=0.1, iters=100, scale=SCALE)
    out.backward(dl)
    assert same_bits(out.detach(), logits) and same_bits(Pg.grad, dP) and same_bits(Xg.grad, dX)
    Pg.grad = None
    ops.ot_match(X, Pg, mu, nu).backward(dl)  # x without grad: no dX launch, the same dP
    assert same_bits(Pg.grad, dP)


def test_no_host_synchronisation(dev):
    from clipfs import ops
    X, P, mu, nu, dl, _, _ = ref_case("caps", "spread", "random", 0.1, 5)  # the forward that asks for more than 64 KB of LDS
    X, P, mu, nu, dl = _to(dev, X, P, mu, nu, dl)
    Xg, Pg = X.clone().requires_grad_(True), P.clone().requires_grad_(True)
    ops.ot_match(Xg, Pg, mu, nu, iters=5).backward(dl)  # warm-up: the allocator
    torch.cuda.synchronize()
    Xg.grad = Pg.grad = None
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = ops.ot_match(Xg, Pg, mu, nu, iters=5)
        out.backward(dl)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(Pg.grad).all()) and bool(torch.isfinite(Xg.grad).all())


def test_refusals_through_ops(dev):
    from clipfs import _lib, ops
    X, P, _, _ = _to(dev, *R.inputs((2, 5, 3, 4, 8)))
    for kw, name in ((dict(eps=0.04), "eps"), (dict(eps=11.0), "eps"), (dict(iters=0), "iters = 0"), (dict(iters=1001), "iters = 1001"),
                     (dict(scale=float("inf")), "scale")):
        with pytest.raises(_lib.ClipfsError, match=name):
            ops.ot_logits(X, P, **kw)
    with pytest.raises(_lib.ClipfsError, match="overlaps"):
        ops.ot_logits(X, P, out=X.view(-1)[:6].view(2, 3))
