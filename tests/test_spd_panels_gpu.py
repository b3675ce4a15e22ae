"""The panelled SPD layer on the GPU (csrc/spd.hip, ops.spd_factor_panels / ops.spd_solve_panels) against the fp64
reference of gda_ref.py on matrices of prescribed spectrum (kappa 10).  The bounds are those of test_spd_gpu.py: the
componentwise backward bound (n + 1) eps sqrt(a_ii a_jj) doubled, the forward bound 8 n eps kappa, the residual bound
(3 n + 2) eps doubled.  The measured fractions are in the table of DESIGN.md section 32."""
import numpy as np
import pytest
import torch

import gda_ref as R
from poison import FILLS, poisoned, same_bits

pytestmark = pytest.mark.gpu
EPS = R.EPS
GUARD = -777.25
KAPPA = 10.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


_CASES = {}


def spd_case(n):
    """(A fp64 of fp32-rounded entries, L fp64): computed once, shared, never written."""
    if n not in _CASES:
        A = R.spd(n, KAPPA)
        _CASES[n] = (A, np.linalg.cholesky(A))
    return _CASES[n]


def _np(t):
    return t.double().cpu().numpy() if t.dtype.is_floating_point else t.cpu().numpy()


def _padded(x, ld, dev, upper=None):
    x = np.array(x, dtype=np.float32)
    if upper is not None:
        x[np.triu_indices(x.shape[0], 1)] = upper
    buf = torch.full((x.shape[0], ld), GUARD, device=dev, dtype=torch.float32)
    buf[:, :x.shape[1]] = torch.from_numpy(x).to(dev)
    return buf, buf[:, :x.shape[1]]


def _check_factor(Ld, A, L64, n, cols=None):
    low = np.tril(Ld)
    k = n if cols is None else cols
    back = float("nan")
    if cols is None:
        back = (np.abs(low @ low.T - A) / np.sqrt(np.outer(np.diag(A), np.diag(A)))).max()
        assert back <= 2 * (n + 1) * EPS, back
    fwd = np.abs(low[:, :k] - L64[:, :k]).max() / np.abs(L64[:, :k]).max() if k else 0.0
    assert fwd <= 8 * n * EPS * KAPPA, fwd
    return back, fwd


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("panel", [32, 64, 128])
@pytest.mark.parametrize("n", [36, 132, 260, 516])
def test_factor(dev, n, panel, pad):
    from clipfs import ops
    A, L64 = spd_case(n)
    ld = n + pad
    runs = []
    for upper in (None,) + FILLS:  # the symmetric input, then its strict upper triangle as 0 / NaN / 1e30
        abuf, a = _padded(A, ld, dev, upper)
        obuf, out = _padded(np.zeros((n, n)), ld, dev)
        chol, info = ops.spd_factor_panels(a, out=out, panel=panel)
        runs.append((chol.contiguous(), info.clone(), obuf, abuf))
    abuf, a = _padded(A, ld, dev, float("nan"))
    inplace, info_in = ops.spd_factor_panels(a, out=a, panel=panel)
    again = ops.spd_factor_panels(_padded(A, ld, dev)[1], panel=panel)[0]
    torch.cuda.synchronize()
    chol, info = runs[0][0], runs[0][1]
    assert int(info.item()) == 0 and int(info_in.item()) == 0
    back, fwd = _check_factor(_np(chol), A, L64, n)
    print(f"factor_panels n {n} panel {panel} ld {ld}: backward {back / (2 * (n + 1) * EPS):.3f} of its bound, "
          f"|L - fp64| {fwd / (8 * n * EPS * KAPPA):.4f} of its bound")
    assert same_bits(chol.t().contiguous(), chol)  # the strict upper triangle is the transpose, bit for bit
    for other, oinfo, obuf, ab in runs[1:]:
        assert same_bits(other, chol) and int(oinfo.item()) == 0
    for _c, _i, obuf, ab in runs:
        if pad:
            assert bool((obuf[:, n:] == GUARD).all()) and bool((ab[:, n:] == GUARD).all())
    assert same_bits(inplace.contiguous(), chol) and same_bits(again, chol)
    if pad:
        assert bool((abuf[:, n:] == GUARD).all())
    if n <= panel:  # a single panel is the fused factor
        assert ops.spd_panels_plan(n, 1, panel)["panels"] == 1
        assert same_bits(ops.spd_factor(_padded(A, ld, dev)[1])[0], chol)


@pytest.mark.parametrize("p", [1, 64, 65, 130])
def test_factor_reports_the_first_bad_pivot_globally(dev, p):
    """A = A0 - delta e_p e_p^T with the fp64 pivot p at -2 % of the diagonal entry: NaN follows column p through every
    later panel, and info must still be p (1-based, global), the columns before it valid, and the calls must return."""
    from clipfs import ops
    n, panel = 132, 64
    A0, L0 = spd_case(n)
    A = A0.copy()
    A[p - 1, p - 1] = R.f32(A0[p - 1, p - 1] - (L0[p - 1, p - 1] ** 2 + 0.02 * A0[p - 1, p - 1]))
    L64, info64 = R.cholesky(A)
    pivot = A[p - 1, p - 1] - L64[p - 1, :p - 1] @ L64[p - 1, :p - 1]
    assert info64 == p and pivot <= -1e-2 * max(abs(A[p - 1, p - 1]), A0[p - 1, p - 1]), (info64, pivot)
    for inplace in (False, True):
        a = torch.from_numpy(A.astype(np.float32)).to(dev)
        chol, info = ops.spd_factor_panels(a, out=a if inplace else None, panel=panel)
        torch.cuda.synchronize()  # the call returns
        assert int(info.item()) == p
        _back, fwd = _check_factor(_np(chol), A, L64, n, cols=p - 1)
        print(f"bad pivot {p} (in place {inplace}): info {int(info.item())}, columns before within {fwd:.2e}")
        x = ops.spd_solve_panels(chol, torch.ones(3, n, device=dev), panel=panel)  # unspecified values, but it returns
        torch.cuda.synchronize()
        assert tuple(x.shape) == (3, n)


def _solve_case(dev, nrhs, n, panel, pad):
    from clipfs import ops
    A, L64 = spd_case(n)
    rng = np.random.default_rng(100 * n + nrhs)
    Rm = R.f32(rng.standard_normal((nrhs, n)))
    X64 = R.solve(L64, Rm)
    chol, info = ops.spd_factor_panels(torch.from_numpy(A.astype(np.float32)).to(dev), panel=panel)
    rbuf, r = _padded(Rm, n + pad, dev)
    xbuf, xo = _padded(np.zeros((nrhs, n)), n + pad, dev)
    x = ops.spd_solve_panels(chol, r, out=xo, panel=panel)
    x4 = ops.spd_solve_panels(chol, r, alpha=4.0, panel=panel)
    xh = ops.spd_solve_panels(chol, r, alpha=0.5, panel=panel)
    fills = []
    for fill in FILLS:  # the output, where the right-hand sides live during the solve, as 0 / NaN / 1e30
        with poisoned(fill):
            fills.append(ops.spd_solve_panels(chol, r, panel=panel))
    inplace = ops.spd_solve_panels(chol, r, out=r, panel=panel)
    torch.cuda.synchronize()
    assert int(info.item()) == 0
    X = _np(x)
    res = np.abs(X @ A - Rm).max()  # rows: x A = r, A symmetric
    bound = 2 * (3 * n + 2) * EPS * (np.abs(A).sum(1).max() * np.abs(X).max() + np.abs(Rm).max())
    fwd = np.abs(X - X64).max() / np.abs(X64).max()
    print(f"solve_panels n {n} panel {panel} nrhs {nrhs}: residual {res / bound:.4f} of its bound, |x - fp64| "
          f"{fwd / (8 * n * EPS * KAPPA):.4f} of its bound")
    assert res <= bound and fwd <= 8 * n * EPS * KAPPA
    xc = x.contiguous()
    assert same_bits(x4, xc * 4.0) and same_bits(xh, xc * 0.5)  # alpha scales exactly for powers of two
    for other in fills:
        assert same_bits(other, xc)
    assert same_bits(inplace.contiguous(), xc)
    if pad:
        assert bool((xbuf[:, n:] == GUARD).all()) and bool((rbuf[:, n:] == GUARD).all())


@pytest.mark.parametrize("n", [132, 260])
@pytest.mark.parametrize("nrhs", [1, 37, 70])
def test_solve(dev, nrhs, n):
    _solve_case(dev, nrhs, n, 64, pad=8 if nrhs == 37 else 0)


def test_the_first_size_the_fused_layer_refuses(dev):
    from clipfs import _lib, ops
    n, panel = 1028, 256
    A, L64 = spd_case(n)
    a = torch.from_numpy(A.astype(np.float32)).to(dev)
    with pytest.raises(_lib.ClipfsError, match="n = 1028"):
        ops.spd_factor(a)
    chol, info = ops.spd_factor_panels(a, panel=panel)
    torch.cuda.synchronize()
    assert int(info.item()) == 0
    back, fwd = _check_factor(_np(chol), A, L64, n)
    print(f"factor_panels n {n} panel {panel}: backward {back / (2 * (n + 1) * EPS):.3f} of its bound, |L - fp64| "
          f"{fwd / (8 * n * EPS * KAPPA):.4f} of its bound")
    assert same_bits(chol.t().contiguous(), chol)
    _solve_case(dev, 37, n, panel, pad=0)
