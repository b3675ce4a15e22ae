"""The SPD layer on the GPU (csrc/spd.hip, ops.spd_factor / ops.spd_solve) against the fp64 reference of gda_ref.py on
matrices of prescribed spectrum.  The bounds are the textbook ones: the componentwise backward bound of a Cholesky factor,
(n + 1) eps sqrt(a_ii a_jj), doubled for the rounding of L itself; the forward bound 8 n eps kappa; the residual bound of
two triangular solves on top of the factor, (3 n + 2) eps, doubled likewise.

Measured on an MI355X (the prints of these tests; the table of DESIGN.md section 30): the componentwise backward error
of the factor is 0.7 to 8.4 eps over the 24 cases (bound 2 (n + 1) eps: at most 17 % of it), L within 2.4e-7 of fp64
relative to max |L| at kappa 10 and 1.0e-6 at kappa 1e3 (bound 8 n eps kappa = 1.9e-5 .. 1.2e-3 at kappa 10); with a
pivot that is not positive the columns before it stay within 1.4e-7; solve residuals at most 0.5 % of their bound, x
within 5.4e-7 of fp64 relative to max |x| at kappa 10 (n up to 1024) and 1.2e-5 at kappa 1e3."""
import numpy as np
import pytest
import torch

import gda_ref as R
from poison import FILLS, same_bits

pytestmark = pytest.mark.gpu
EPS = R.EPS
GUARD = -777.25


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


_CASES = {}


def spd_case(n, kappa):
    """(A fp64 of fp32-rounded entries, L fp64, max |L|): computed once, shared, never written."""
    if (n, kappa) not in _CASES:
        A = R.spd(n, kappa)
        L, info = R.cholesky(A)
        assert info == 0
        _CASES[(n, kappa)] = (A, L)
    return _CASES[(n, kappa)]


def _np(t):
    return t.double().cpu().numpy() if t.dtype.is_floating_point else t.cpu().numpy()


def _padded(x, ld, dev, upper=None):
    """[rows, ld] device buffer filled with GUARD holding x in its first columns; returns (buffer, view).  ``upper``: the
    fill of the strict upper triangle of a square x."""
    x = np.array(x, dtype=np.float32)
    if upper is not None:
        x[np.triu_indices(x.shape[0], 1)] = upper
    buf = torch.full((x.shape[0], ld), GUARD, device=dev, dtype=torch.float32)
    buf[:, :x.shape[1]] = torch.from_numpy(x).to(dev)
    return buf, buf[:, :x.shape[1]]


def _check_factor(Ld, A, L64, n, kappa, cols=None):
    """The bounds on a device factor (fp64 copy of the n x n output); ``cols``: only the first ``cols`` columns."""
    low = np.tril(Ld)
    k = n if cols is None else cols
    scale = np.sqrt(np.outer(np.diag(A), np.diag(A)))
    if cols is None:
        back = (np.abs(low @ low.T - A) / scale).max()
        assert back <= 2 * (n + 1) * EPS, back
    else:
        back = float("nan")
    fwd = np.abs(low[:, :k] - L64[:, :k]).max() / np.abs(L64[:, :k]).max() if k else 0.0
    if kappa == 10.0:
        assert fwd <= 8 * n * EPS * kappa, fwd
    return back, fwd


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("kappa", [10.0, 1e3])
@pytest.mark.parametrize("n", [4, 32, 36, 64, 132, 260])
def test_factor(dev, n, kappa, pad):
    from clipfs import ops
    A, L64 = spd_case(n, kappa)
    ld = n + pad
    runs = []
    for upper in (None,) + FILLS:  # the symmetric input, then its strict upper triangle as 0 / NaN / 1e30
        abuf, a = _padded(A, ld, dev, upper)
        obuf, out = _padded(np.zeros((n, n)), ld, dev)
        chol, info = ops.spd_factor(a, out=out)
        runs.append((chol.contiguous(), info.clone(), obuf, abuf))
    abuf, a = _padded(A, ld, dev, float("nan"))
    inplace, info_in = ops.spd_factor(a, out=a)
    again = ops.spd_factor(_padded(A, ld, dev)[1])[0]  # a second run, into a fresh contiguous output
    torch.cuda.synchronize()
    chol, info = runs[0][0], runs[0][1]
    assert int(info.item()) == 0 and int(info_in.item()) == 0
    Ld = _np(chol)
    back, fwd = _check_factor(Ld, A, L64, n, kappa)
    print(f"factor n {n} kappa {kappa:g} ld {ld}: backward {back / EPS:.2f} eps (bound {2 * (n + 1)}), "
          f"|L - fp64| {fwd:.2e} of max |L| (bound {8 * n * EPS * kappa:.2e})")
    iu = np.triu_indices(n, 1)
    assert same_bits(chol.t().contiguous(), chol)  # the strict upper triangle is the transpose of the lower, bit for bit
    assert np.array_equal(Ld[iu], Ld.T[iu])
    for other, oinfo, obuf, ab in runs[1:]:
        assert same_bits(other, chol) and int(oinfo.item()) == 0
    for _c, _i, obuf, ab in runs:
        if pad:
            assert bool((obuf[:, n:] == GUARD).all()) and bool((ab[:, n:] == GUARD).all())  # guard columns keep their fill
    assert same_bits(inplace.contiguous(), chol) and same_bits(again, chol)
    if pad:
        assert bool((abuf[:, n:] == GUARD).all())


@pytest.mark.parametrize("p", [1, 32, 33, 68])
def test_factor_reports_the_first_pivot_that_is_not_positive(dev, p):
    """A = L0 L0^T - delta e_p e_p^T with delta chosen so that the fp64 pivot p is -2 % of the diagonal entry: the error
    path stores NaN values after column p and must report p, keep the columns before it, and return."""
    from clipfs import ops
    n, kappa = 68, 10.0
    A0, L0 = spd_case(n, kappa)
    A = A0.copy()
    A[p - 1, p - 1] = R.f32(A0[p - 1, p - 1] - (L0[p - 1, p - 1] ** 2 + 0.02 * A0[p - 1, p - 1]))
    L64, info64 = R.cholesky(A)
    pivot = A[p - 1, p - 1] - L64[p - 1, :p - 1] @ L64[p - 1, :p - 1]
    assert info64 == p and pivot <= -1e-2 * max(abs(A[p - 1, p - 1]), A0[p - 1, p - 1]), (info64, pivot)
    for inplace in (False, True):
        a = torch.from_numpy(A.astype(np.float32)).to(dev)
        chol, info = ops.spd_factor(a, out=a if inplace else None)
        torch.cuda.synchronize()  # the call returns
        assert int(info.item()) == p
        _back, fwd = _check_factor(_np(chol), A, L64, n, kappa, cols=p - 1)
        print(f"not positive definite at {p} (in place {inplace}): info {int(info.item())}, columns before within {fwd:.2e}")
        # what a solve makes of such a factor is unspecified, but it returns
        x = ops.spd_solve(chol, torch.ones(3, n, device=dev))
        torch.cuda.synchronize()
        assert tuple(x.shape) == (3, n)


@pytest.mark.parametrize("kappa", [10.0, 1e3])
@pytest.mark.parametrize("n", [36, 132])
@pytest.mark.parametrize("nrhs", [1, 5, 37, 70])
def test_solve(dev, nrhs, n, kappa):
    from clipfs import ops
    _solve_case(dev, nrhs, n, kappa, pad=8 if nrhs == 37 else 0)


@pytest.mark.parametrize("n,nrhs", [(516, 37), (1024, 5)])
def test_factor_and_solve_where_the_rows_need_more_than_64_kb_of_lds(dev, n, nrhs):
    from clipfs import ops
    A, L64 = spd_case(n, 10.0)
    chol, info = ops.spd_factor(torch.from_numpy(A.astype(np.float32)).to(dev))
    assert int(info.item()) == 0
    back, fwd = _check_factor(_np(chol), A, L64, n, 10.0)
    print(f"factor n {n}: backward {back / EPS:.2f} eps (bound {2 * (n + 1)}), |L - fp64| {fwd:.2e}")
    assert ops.spd_plan(n, nrhs)["solve_lds_bytes"] > 64 * 1024
    _solve_case(dev, nrhs, n, 10.0, pad=0)


def _solve_case(dev, nrhs, n, kappa, pad):
    from clipfs import ops
    A, L64 = spd_case(n, kappa)
    rng = np.random.default_rng(100 * n + nrhs)
    Rm = R.f32(rng.standard_normal((nrhs, n)))
    X64 = R.solve(L64, Rm)
    chol, info = ops.spd_factor(torch.from_numpy(A.astype(np.float32)).to(dev))
    rbuf, r = _padded(Rm, n + pad, dev)
    xbuf, xo = _padded(np.zeros((nrhs, n)), n + pad, dev)
    x = ops.spd_solve(chol, r, out=xo)
    x4 = ops.spd_solve(chol, r, alpha=4.0)
    xh = ops.spd_solve(chol, r, alpha=0.5)
    again = ops.spd_solve(chol, r)
    inplace = ops.spd_solve(chol, r, out=r)
    torch.cuda.synchronize()
    assert int(info.item()) == 0
    X = _np(x)
    res = np.abs(X @ A - Rm).max()  # rows: x A = r, A symmetric
    bound = 2 * (3 * n + 2) * EPS * (np.abs(A).sum(1).max() * np.abs(X).max() + np.abs(Rm).max())
    fwd = np.abs(X - X64).max() / np.abs(X64).max()
    print(f"solve n {n} nrhs {nrhs} kappa {kappa:g}: residual {res:.2e} (bound {bound:.2e}), |x - fp64| {fwd:.2e} of max |x| "
          f"(bound {8 * n * EPS * kappa:.2e} at kappa 10)")
    assert res <= bound
    if kappa == 10.0:
        assert fwd <= 8 * n * EPS * kappa
    xc = x.contiguous()
    assert same_bits(x4, xc * 4.0) and same_bits(xh, xc * 0.5)  # alpha scales exactly for powers of two
    assert same_bits(again, xc) and same_bits(inplace.contiguous(), xc)
    if pad:
        assert bool((xbuf[:, n:] == GUARD).all()) and bool((rbuf[:, n:] == GUARD).all())
