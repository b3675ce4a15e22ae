"""The kernel ridge reference (krr_ref.py) against numpy's own solver, its exact identity, the condition caps the GPU
tests rely on, and the host-only plans' closed forms (no GPU: the plans open no device)."""
import numpy as np
import pytest

import krr_ref as R

CASES = [(shape, k) for shape in R.SHAPES for k in range(len(R.SETTINGS))]
_REFS = {}


def ref_case(shape, k, with_base=True):
    """(geo, base_S, ref) for SHAPES entry ``shape`` at SETTINGS[k]: computed once, shared, never written."""
    key = (shape, k, with_base)
    if key not in _REFS:
        n, d, C = shape
        geo = R.shots(n, d, C)
        base_S = R.base_of(geo, geo["S"]) if with_base else None
        beta, lam = R.SETTINGS[k]
        _REFS[key] = (geo, base_S, R.fit(geo["S"], geo["labels"], C, base_S, beta, lam))
    return _REFS[key]


@pytest.mark.parametrize("shape,k", CASES)
def test_caps_solver_and_identity(shape, k):
    geo, base_S, ref = ref_case(shape, k)
    n, d, C = shape
    assert not np.array_equal(geo["labels"], np.sort(geo["labels"])) or C == 1  # unsorted on purpose
    assert np.abs(np.linalg.norm(geo["S"], axis=1) - 1).max() < 1e-6
    print(f"n {n} d {d} C {C} beta {ref['beta']:g} lambda {ref['lam']:g}: cond {ref['cond']:.1f} (cap {R.COND_CAPS[k]:g})")
    assert ref["cond"] <= R.COND_CAPS[k]
    direct = np.linalg.solve(ref["A"], ref["Et"].T).T
    assert np.abs(direct - ref["At"]).max() <= 1e-11 * ref["cond"] * np.abs(direct).max()
    assert not ref["At"][:, n:].any() and not ref["Et"][:, n:].any()  # the pad solves to 0
    # the exact identity: k(S, S) At^T = (A - lambda I) At^T = Et^T - lambda At^T
    lhs = R.apply(geo["S"], geo["S"], ref["At"], base_S, ref["beta"]) - base_S
    rhs = (ref["Et"] - ref["lam"] * ref["At"])[:, :n].T
    assert np.abs(lhs - rhs).max() <= 1e-11 * ref["cond"] * max(1.0, np.abs(rhs).max())


def test_rule_pieces():
    geo = R.shots(37, 64, 5)
    A = R.system(geo["S"], 2.0, 0.5)
    assert A.shape == (40, 40) and np.array_equal(A[37:, 37:], np.eye(3)) and not A[37:, :37].any() and not A[:37, 37:].any()
    assert np.allclose(np.diag(A)[:37], 1.5, atol=1e-6)  # unit rows: exp(0) + lambda
    Et = R.targets(geo["labels"], 5, None, 2.0)
    assert Et.shape == (5, 40) and Et.sum() == 2.0 * 37 and Et[geo["labels"][7], 7] == 2.0
    base = R.base_of(geo, geo["S"])
    assert np.array_equal(R.targets(geo["labels"], 5, base, 2.0)[:, :37], Et[:, :37] - base.T)
    X, target, b = R.queries(geo, 9)
    assert np.allclose(R.apply(X, geo["S"], np.zeros((5, 40)), b, 1.0), b)


def _panels_closed_form(n, panel):
    P = -(-n // panel)
    launches = gemms = 0
    for k in range(P):
        pn = min(panel, n - k * panel)
        rest = n - k * panel - pn
        launches += -(-pn // 32) + (2 if rest else 0)
        gemms += -(-rest // (4 * panel))
    return P, launches, gemms


@pytest.mark.parametrize("n,panel", [(36, 64), (132, 64), (260, 32), (516, 128), (1028, 256), (6352, 256), (16000, 512),
                                     (16384, 1024), (16384, 32)])
def test_spd_panels_plan_closed_forms(n, panel):
    from clipfs import ops
    for nrhs in (1, 1000):
        p = ops.spd_panels_plan(n, nrhs, panel)
        P, launches, gemms = _panels_closed_form(n, panel)
        assert (p["panel"], p["panels"], p["band"]) == (panel, P, 4 * panel)
        assert (p["factor_launches"], p["factor_gemms"]) == (launches, gemms)
        assert (p["solve_launches"], p["solve_gemms"]) == (2 * P + 1, 2 * (P - 1))
        assert p["threads"] == 256
        assert p["lds_bytes"] == max(4 * (32 * (min(n, panel) + 4) + 6 * 32 * 33), 4 * 10 * 32 * 33 + 4) <= 160 * 1024
    if n <= panel:  # a single panel: the launches of ops.spd_factor
        assert p["factor_launches"] == ops.spd_plan(n)["factor_launches"] and p["factor_gemms"] == 0


@pytest.mark.parametrize("n,C,B", [(1, 1, 1), (37, 3, 33), (132, 128, 70), (130, 129, 1), (260, 256, 5), (516, 257, 64),
                                   (1024, 1024, 8192), (1028, 1025, 8192), (16000, 4096, 100)])
def test_krr_plan_closed_forms(n, C, B):
    from clipfs import ops
    panel, d = 256, 512
    p = ops.krr_plan(n, C, d, B, panel)
    n4 = R.n4_of(n)
    assert p["n4"] == n4 and p["panelled"] == int(n4 > 1024)
    if n4 > 1024:
        sp = ops.spd_panels_plan(n4, C, panel)
        factor, solve = sp["factor_launches"] + sp["factor_gemms"], sp["solve_launches"] + sp["solve_gemms"]
    else:
        sp = ops.spd_plan(n4, C)
        factor, solve = sp["factor_launches"], 2
    assert (p["factor_launches"], p["solve_launches"], p["fit_launches"]) == (factor, solve, 3 + factor + solve)
    tiles = -(-(-(-C // 32)) // 4)
    nt = 1 if tiles <= 1 else 2 if tiles <= 2 else 4 if tiles <= 4 else 8
    assert (p["tiles_per_wave"], p["class_chunk"]) == (nt, 128 * nt)
    assert (p["apply_grid_x"], p["apply_grid_y"], p["threads"]) == (-(-B // 32), -(-C // (128 * nt)), 256)
    assert 54784 <= p["lds_bytes"] <= 160 * 1024
