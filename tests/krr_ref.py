"""The kernel ridge rule of include/clipfs.h ("KRR") in numpy fp64, from fp32-rounded inputs: the reference of
test_krr_cpu.py, test_spd_panels_gpu.py and test_krr_gpu.py.  Nothing here imports the package.

    shots(n, d, C)      the seeded few-shot set: unit rows around unit class centres, labels j mod C (UNSORTED on purpose)
    queries(geo, B)     unit queries near the centres, their targets and zero-shot-like base logits
    fit(...)            A (pad = identity), Et, L, At and cond(A) of the rule
    apply(...)          base + k(X, S) At[:, :n]^T
    the error bounds    what fp32 may cost, from the precision and the shapes (each derived where it is defined)
"""
import numpy as np

EPS = 2.0 ** -24
SETTINGS = ((5.5, 1.0), (5.5, 0.1), (1.0, 1.0))  # (beta, lambda)
COND_CAPS = (25.0, 25.0, 400.0)                   # asserted in fp64 before any accuracy check
SHAPES = ((36, 64, 3), (132, 64, 37), (260, 132, 37), (516, 64, 130), (1028, 128, 64))  # (n, d, C)


def f32(x):
    """x rounded to fp32, as float64."""
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def unit_rows(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def n4_of(n):
    return (n + 3) // 4 * 4


_SHOTS = {}


def shots(n, d, C, seed=0):
    """dict(S [n, d] fp32-rounded unit rows, labels [n] = j mod C, centres [C, d], n, d, C): computed once, never written."""
    key = (n, d, C, seed)
    if key not in _SHOTS:
        rng = np.random.default_rng(7000 + 13 * n + d + seed)
        centres = unit_rows(rng.standard_normal((C, d)))
        labels = np.arange(n) % C
        S = f32(unit_rows(centres[labels] + 0.5 * rng.standard_normal((n, d)) / np.sqrt(d)))
        _SHOTS[key] = dict(S=S, labels=labels, centres=centres, n=n, d=d, C=C)
    return _SHOTS[key]


def queries(geo, B, seed=0, noise=0.5, scale=1.0):
    """(X [B, d] fp32-rounded unit rows near the centres, target [B], base [B, C] fp32-rounded = scale X T^T for class
    features T = the centres seen through some noise)."""
    rng = np.random.default_rng(8000 + seed)
    C, d = geo["C"], geo["d"]
    target = rng.integers(0, C, size=B)
    X = f32(unit_rows(geo["centres"][target] + noise * rng.standard_normal((B, d)) / np.sqrt(d)))
    T = unit_rows(geo["centres"] + 0.5 * rng.standard_normal((C, d)) / np.sqrt(d))
    return X, target, f32(scale * X @ T.T)


def base_of(geo, X, seed=0, scale=1.0):
    """Base logits of any unit rows X (the shots themselves included), from the same noisy class features as queries()."""
    rng = np.random.default_rng(8500 + seed)
    T = unit_rows(geo["centres"] + 0.5 * rng.standard_normal((geo["C"], geo["d"])) / np.sqrt(geo["d"]))
    return f32(scale * np.asarray(X, dtype=np.float64) @ T.T)


def kernel(X, S, beta):
    return np.exp(-beta * (1.0 - np.asarray(X, dtype=np.float64) @ np.asarray(S, dtype=np.float64).T))


def system(S, beta, lam):
    """A [n4, n4]: the kernel matrix + lam I in [n, n], the identity in the pad."""
    n = S.shape[0]
    A = np.eye(n4_of(n))
    A[:n, :n] = kernel(S, S, beta) + lam * np.eye(n)
    return A


def targets(labels, C, base_S, t):
    """Et [C, n4]: Et[c, j] = t [labels[j] == c] - base_S[j, c], pad columns 0."""
    n = len(labels)
    Et = np.zeros((C, n4_of(n)))
    Et[labels, np.arange(n)] = t
    if base_S is not None:
        Et[:, :n] -= np.asarray(base_S, dtype=np.float64).T
    return Et


def solve_rows(L, R):
    """Rows of R as right-hand sides: X[i] = (L L^T)^-1 R[i]."""
    Y = np.linalg.solve(L, np.asarray(R, dtype=np.float64).T)
    return np.linalg.solve(L.T, Y).T


def fit(S, labels, C, base_S=None, beta=5.5, lam=1.0, t=1.0):
    beta, lam, t = float(np.float32(beta)), float(np.float32(lam)), float(np.float32(t))
    A = system(S, beta, lam)
    Et = targets(labels, C, base_S, t)
    L = np.linalg.cholesky(A)
    At = solve_rows(L, Et)
    ev = np.linalg.eigvalsh(A)
    return dict(A=A, Et=Et, L=L, At=At, cond=float(ev[-1] / ev[0]), n=S.shape[0], n4=A.shape[0], d=S.shape[1], C=C, beta=beta,
                lam=lam, t=t)


def apply(X, S, At, base, beta):
    n = S.shape[0]
    out = kernel(X, S, float(np.float32(beta))) @ At[:, :n].T
    return out if base is None else base + out


# ---------------------------------------------------------------------------------------------------- error bounds
def g_rel(d, beta):
    """Relative error of one kernel value: (d + 2) eps beta on the exponent (a d-term fp32 dot product of unit rows, the
    subtraction of 1, the product with beta log2 e), and 3 eps for exp2 itself and one more rounding."""
    return ((d + 2) * beta + 3) * EPS


def system_bound(ref):
    """[n4, n4]: g_rel of every element (the diagonal's + lambda included); the pad is exact."""
    b = g_rel(ref["d"], ref["beta"]) * np.abs(ref["A"])
    b[ref["n"]:, :] = 0.0
    b[:, ref["n"]:] = 0.0
    return b


def targets_bound(ref, base_S):
    """[C, n4]: one rounding of the subtraction (t and base_S are fp32 inputs); exact without a base."""
    return EPS * np.abs(ref["Et"]) if base_S is not None else np.zeros_like(ref["Et"])


def factor_bound(A):
    """Componentwise backward bound of a Cholesky factor, (n + 1) eps sqrt(a_ii a_jj), doubled for the rounding of L."""
    n = A.shape[0]
    return 2 * (n + 1) * EPS * np.sqrt(np.outer(np.diag(A), np.diag(A)))


def residual_bound(A, X, R):
    """max |X A - R| of two triangular solves on top of the factor: (3 n + 2) eps, doubled."""
    n = A.shape[0]
    return 2 * (3 * n + 2) * EPS * (np.abs(A).sum(1).max() * np.abs(X).max() + np.abs(R).max())


def solution_bound(n, cond, X):
    """Forward bound of the solution: 8 n eps cond of max |X|."""
    return 8 * n * EPS * cond * np.abs(X).max()


def at_bound(ref):
    """Per entry of At from a fit: the solve's forward bound 8 n4 eps cond and the system's relative error g_rel (its
    entries are positive, so the relative perturbation of A is at most that), doubled, amplified by cond."""
    return (8 * ref["n4"] + 2 * ((ref["d"] + 2) * ref["beta"] + 3)) * EPS * ref["cond"] * np.abs(ref["At"]).max()


def apply_bound(X, S, At, base, beta, d):
    """[B, C]: (d + 2) eps beta on the exponent plus (n + 2) eps on the sum, times sum_j |g_j At[c, j]|; one rounding of
    the base's addition."""
    n = S.shape[0]
    mag = kernel(X, S, beta) @ np.abs(At[:, :n]).T
    b = ((d + 2) * beta + n + 2) * EPS * mag
    return b if base is None else b + EPS * np.abs(base)


def logit_bound(ref, X, S, base):
    """[B, C]: the head's logits from a fit: at_bound carried through the kernel row sums, and apply_bound."""
    return kernel(X, S, ref["beta"]).sum(1)[:, None] * at_bound(ref) + apply_bound(X, S, ref["At"], base, ref["beta"], ref["d"])


def hits(logits, target):
    """Top-1 hits, the lowest index on ties (numpy's rule)."""
    return int((np.argmax(logits, axis=1) == target).sum())
