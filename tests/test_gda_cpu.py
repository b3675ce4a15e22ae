"""The GDA rule and the plans of the SPD layer without a GPU: the fp64 reference (gda_ref.py) agrees with the published
explicit form and with the LDA discriminant, the plans' closed forms hold, and the pinned geometries meet the condition
and margin requirements the GPU tests rely on (asserted there again before the device is touched)."""
import numpy as np
import pytest

import gda_ref as R

GEOS = tuple(R.GEOMETRIES)
# (geometry, rows, seed) of the alpha search: every row and every cell of the default grid keeps 64 error bounds between
# its best and its second class in fp64
SEARCH_CASES = (("G0", 40, 0), ("G1", 40, 0), ("G2", 70, 0))
SHRINK_GEOS = ("G1", "G2")
SHRINKS = (0.5, 1.0, 4.0)
MARGIN = 64.0
COND_MAX = 10.0
_REF = {}


def ref_case(name, shrink=1.0, prior="uniform"):
    """(geometry, fp64 fit) computed once, shared, never written."""
    key = (name, shrink, prior)
    if key not in _REF:
        geo = R.geometry(name)
        _REF[key] = (geo, R.fit(geo["S"], geo["offsets"], shrink, prior))
    return _REF[key]


def assert_search_margins(name, B, seed, alphas=R.DEFAULT_ALPHAS):
    geo, ref = ref_case(name)
    F, target, base = R.eval_set(geo, B, seed)
    ratio = R.margin_ratio(ref, F, base, alphas)
    assert ratio >= MARGIN, (name, B, seed, ratio)
    return geo, ref, F, target, base


@pytest.mark.parametrize("name", GEOS)
def test_reference_is_the_published_explicit_form(name):
    geo, ref = ref_case(name)
    M, d = geo["M"], geo["d"]
    assert np.array_equal(np.diff(geo["offsets"]), geo["counts"]) and geo["counts"].min() >= 1
    assert np.abs(np.linalg.norm(geo["S"], axis=1) - 1).max() < 1e-6
    X = geo["S"] - ref["mu"][geo["labels"]]
    Sigma = X.T @ X / (M - 1)
    W = d * (np.linalg.pinv((M - 1) * Sigma + np.trace(Sigma) * np.eye(d)) @ ref["mu"].T).T
    assert np.abs(W - ref["W"]).max() <= 1e-12 * np.abs(W).max()
    assert ref["info"] == 0 and np.abs(ref["L"] @ ref["L"].T - ref["A"]).max() <= 1e-13 * np.abs(ref["A"]).max()


@pytest.mark.parametrize("name", GEOS)
@pytest.mark.parametrize("prior", ["uniform", "empirical"])
def test_reference_is_the_lda_discriminant_up_to_a_row_constant(name, prior):
    """log pi_c - 1/2 (f - mu_c)^T P (f - mu_c) with P = d A^-1 equals f W_c + b_c - 1/2 f^T P f: the last term does not
    depend on the class."""
    geo, ref = ref_case(name, 1.0, prior)
    F = R.eval_set(geo, 9, 4)[0]
    P = geo["d"] * np.linalg.inv(ref["A"])
    diff = F[:, None, :] - ref["mu"][None, :, :]
    lda = ref["logpi"][None, :] - 0.5 * np.einsum("bcd,de,bce->bc", diff, P, diff)
    rest = lda - R.scores(F, ref["W"], ref["b"])
    assert np.abs(rest - rest[:, :1]).max() <= 1e-10 * np.abs(lda).max()
    if prior == "empirical":
        assert np.allclose(np.exp(ref["logpi"]), geo["counts"] / geo["M"])


def test_unblocked_cholesky_reports_the_first_bad_pivot():
    A = R.spd(12, 10.0)
    L, info = R.cholesky(A)
    assert info == 0 and np.abs(L @ L.T - A).max() < 1e-14 and np.array_equal(L, np.tril(L))
    B = A.copy()
    B[np.triu_indices(12, 1)] = np.nan  # only the lower triangle is read
    assert np.array_equal(R.cholesky(B)[0], L)
    for p in (1, 5, 12):
        Bad = A.copy()
        Bad[p - 1, p - 1] -= 2.0
        Lb, info = R.cholesky(Bad)
        assert info == p and np.array_equal(Lb[:, :p - 1], L[:, :p - 1]) and np.isnan(Lb[p - 1, p - 1])
    X = R.solve(L, np.eye(12)[:5])
    assert np.abs(A @ X.T - np.eye(12)[:, :5]).max() < 1e-13


@pytest.mark.parametrize("kappa", [10.0, 1e3])
def test_spd_matrices_have_the_prescribed_spectrum(kappa):
    for n in (4, 36, 132):
        A = R.spd(n, kappa)
        ev = np.linalg.eigvalsh(A)
        assert np.array_equal(A, A.T) and abs(ev[-1] / ev[0] / kappa - 1) < 1e-3


def test_plans_closed_forms():
    from clipfs import ops
    for n in (4, 36, 512, 1024):
        for nrhs in (1, 37, 1000, 65536):
            p = ops.spd_plan(n, nrhs)
            assert p["factor_launches"] == -(-n // 32) == p["factor_grid"] and p["solve_launches"] == 2 and p["block"] == 32
            assert p["solve_grid"] == -(-nrhs // 32) and p["threads"] == 256
            assert p["lds_bytes"] == max(p["factor_lds_bytes"], p["solve_lds_bytes"]) <= 160 * 1024
            assert p["solve_lds_bytes"] >= 32 * n * 4  # the 32 right-hand-side rows live on chip
        counts = {(M, C): ops.gda_plan(M, C, n)["launches"] for M, C in ((2, 1), (70, 5), (16000, 1000), (65536, 4096))}
        assert set(counts.values()) == {6 + -(-n // 32)}, counts  # a function of n alone
        g = ops.gda_plan(16000, 1000, n)
        assert g["Mp"] == 16000 and g["xt_floats"] == n * 16000 and g["lds_bytes"] <= 160 * 1024
        assert g["factor_launches"] == -(-n // 32) and g["solve_launches"] == 2 and g["solve_grid"] == 32
    assert ops.gda_plan(33, 5, 64)["Mp"] == 64 and ops.gda_plan(32, 5, 64)["Mp"] == 32
    assert ops.GDA_DEFAULT_ALPHAS == R.DEFAULT_ALPHAS


def test_pinned_geometries_are_well_conditioned():
    for name in GEOS:
        assert ref_case(name)[1]["cond"] <= COND_MAX, name
    for name in SHRINK_GEOS:
        for s in SHRINKS:
            assert ref_case(name, s)[1]["cond"] <= COND_MAX, (name, s)
    # the fp32 restatement of W stays well inside its bound on every geometry
    for name in GEOS:
        geo, ref = ref_case(name)
        A32 = ref["A"].astype(np.float32)
        L32 = np.linalg.cholesky(A32.astype(np.float64)).astype(np.float32).astype(np.float64)
        W32 = geo["d"] * R.solve(L32, ref["mu"].astype(np.float32))
        assert np.abs(W32 - ref["W"]).max() <= R.w_bound(ref)


@pytest.mark.parametrize("name,B,seed", SEARCH_CASES)
def test_search_margins_hold_on_the_pinned_seeds(name, B, seed):
    geo, ref, F, target, base = assert_search_margins(name, B, seed)
    h = R.hits(R.scores(F, ref["W"], ref["b"]), base, R.DEFAULT_ALPHAS, target)
    assert h.shape == (9,) and h.max() <= B
    if name == "G0":
        assert len(set(h.tolist())) > 1  # a case where the cells differ, so that the choice of alpha means something
