"""The GDA rule of include/clipfs.h ("GDA") and the SPD layer under it in numpy fp64, from fp32-rounded inputs: the
reference of test_gda_cpu.py, test_spd_gpu.py and test_gda_gpu.py.  Nothing here imports the package.

    geometry(name)      the seeded few-shot sets G0 .. G3: unit shots around unit class centres, sorted by class
    fit(...)            steps 1-6: mu, xt, G, tau, A, L, W, b (and cond(A))
    cholesky(A)         unblocked, lower triangle only, reporting the first pivot <= 0 or not finite (1-based)
    spd(n, kappa)       Q diag(geomspace(1, 1 / kappa)) Q^T, rounded to fp32 and symmetric bit for bit
    the error bounds    w_bound, b_bound, g_bound, logit_bound: what fp32 may cost, from the precision and the shapes
"""
import numpy as np

EPS = 2.0 ** -24
GEOMETRIES = {  # name: (C, d, counts or None = 1-5 drawn by the seed, seed)
    "G0": (3, 4, (2, 2, 3), 0),
    "G1": (5, 36, (1, 2, 3, 4, 5), 1),
    "G2": (37, 132, None, 2),
    "G3": (70, 64, None, 3),
}
DEFAULT_ALPHAS = tuple(10.0 ** e for e in range(-4, 5))


def f32(x):
    """x rounded to fp32, as float64."""
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def unit_rows(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def geometry(name, noise=1.0):
    """dict(S [M, d] fp32-rounded unit rows sorted by class, labels [M], offsets int32 [C + 1], counts, centres [C, d], C, d, M)."""
    C, d, counts, seed = GEOMETRIES[name]
    rng = np.random.default_rng(1000 + seed)
    counts = np.asarray(counts if counts is not None else rng.integers(1, 6, size=C), dtype=np.int64)
    centres = unit_rows(rng.standard_normal((C, d)))
    labels = np.repeat(np.arange(C), counts)
    S = f32(unit_rows(centres[labels] + noise * rng.standard_normal((labels.size, d)) / np.sqrt(d)))
    offsets = np.zeros(C + 1, dtype=np.int32)
    offsets[1:] = np.cumsum(counts)
    return dict(S=S, labels=labels, offsets=offsets, counts=counts, centres=centres, C=C, d=d, M=int(labels.size))


def eval_set(geo, B, seed, noise=0.25, scale=100.0):
    """(F [B, d] fp32-rounded unit rows near the centres, target [B], base [B, C] fp32-rounded = scale F T^T for class
    features T = the centres seen through some noise)."""
    rng = np.random.default_rng(5000 + seed)
    C, d = geo["C"], geo["d"]
    target = rng.integers(0, C, size=B)
    F = f32(unit_rows(geo["centres"][target] + noise * rng.standard_normal((B, d)) / np.sqrt(d)))
    T = unit_rows(geo["centres"] + 0.5 * rng.standard_normal((C, d)) / np.sqrt(d))
    return F, target, f32(scale * F @ T.T)


def cholesky(A):
    """(L, info): the unblocked Cholesky factor from the lower triangle of A.  info = 0, or the 1-based index of the first
    pivot that is <= 0 or not finite; then the columns before it are valid and the rest of L is NaN."""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    L = np.zeros((n, n))
    for k in range(n):
        p = A[k, k] - L[k, :k] @ L[k, :k]
        if not (p > 0 and np.isfinite(p)):
            L[k:, k:] = np.nan
            L[np.triu_indices(n, 1)] = 0.0
            return L, k + 1
        L[k, k] = np.sqrt(p)
        L[k + 1:, k] = (A[k + 1:, k] - L[k + 1:, :k] @ L[k, :k]) / L[k, k]
    return L, 0


def solve(L, R):
    """Rows of R as right-hand sides: X[i] = (L L^T)^-1 R[i]."""
    Y = np.linalg.solve(L, np.asarray(R, dtype=np.float64).T)
    return np.linalg.solve(L.T, Y).T


def spd(n, kappa, seed=0):
    """Q diag(geomspace(1, 1 / kappa, n)) Q^T with a seeded orthogonal Q, rounded to fp32, exactly symmetric."""
    rng = np.random.default_rng(9000 + 7 * n + seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = f32((Q * np.geomspace(1.0, 1.0 / kappa, n)) @ Q.T)
    A = np.tril(A) + np.tril(A, -1).T
    return A


def fit(S, offsets, shrink=1.0, prior="uniform"):
    """Steps 1-6 in fp64 from the fp32-rounded shots."""
    S = np.asarray(S, dtype=np.float64)
    M, d = S.shape
    C = len(offsets) - 1
    counts = np.diff(offsets).astype(np.int64)
    assert (counts >= 1).all() and M >= 2
    labels = np.repeat(np.arange(C), counts)
    mu = np.stack([S[offsets[c]:offsets[c + 1]].sum(0) / counts[c] for c in range(C)])
    X = S - mu[labels]
    Mp = (M + 31) // 32 * 32
    xt = np.zeros((d, Mp))
    xt[:, :M] = X.T
    G = xt @ xt.T
    tau = float(np.trace(G))
    A = G + shrink * tau / (M - 1) * np.eye(d)
    L, info = cholesky(A)
    W = d * solve(L, mu) if info == 0 else np.full((C, d), np.nan)
    logpi = np.full(C, -np.log(C)) if prior == "uniform" else np.log(counts / M)
    b = logpi - 0.5 * np.einsum("cd,cd->c", mu, W)
    ev = np.linalg.eigvalsh(A)
    return dict(mu=mu, xt=xt, G=G, tau=tau, A=A, L=L, info=info, W=W, b=b, cond=float(ev[-1] / ev[0]), M=M, d=d, C=C,
                counts=counts, logpi=logpi)


def scores(F, W, b):
    return np.asarray(F, dtype=np.float64) @ W.T + b


def logits(F, W, b, base, alpha):
    g = scores(F, W, b)
    return alpha * g if base is None else base + alpha * g


def argmax_low(x):
    """Row argmax, the lowest index on ties (numpy's rule)."""
    return np.argmax(x, axis=1)


def hits(g, base, alphas, target):
    base = 0.0 if base is None else base
    return np.array([(argmax_low(base + a * g) == target).sum() for a in alphas], dtype=np.int64)


# ---------------------------------------------------------------------------------------------------- error bounds
def w_bound(ref):
    """Per entry of W: (8 d + 2 M) 2^-24 cond(A) max |W| -- the solve's backward error 8 d eps and the Gram product's
    2 M eps (its M-term sums and the centring), each amplified by cond(A)."""
    return (8 * ref["d"] + 2 * ref["M"]) * EPS * ref["cond"] * np.abs(ref["W"]).max()


def b_bound(ref):
    """Per class, from the W bound: b_c = log pi_c - 1/2 mu_c . W_c with mu_c off by n_c eps per entry, W_c by w_bound, a
    d-term fp32 dot product ((d + 1) eps of sum |mu| |W|), and the roundings of log pi_c, the half product and the sum."""
    mu, W = np.abs(ref["mu"]), np.abs(ref["W"])
    dot = (mu * W).sum(1)
    return (0.5 * (mu.sum(1) * w_bound(ref) + ref["counts"] * EPS * W.sum(1) + (ref["d"] + 1) * EPS * dot)
            + 2 * EPS * (np.abs(ref["logpi"]) + 0.5 * dot + np.abs(ref["b"])))


def g_bound(ref, F):
    """[B, C]: the error of g = F W^T + b: |f|_1 w_bound, the (d + 1)-term fp32 sum, b_bound."""
    F = np.abs(np.asarray(F, dtype=np.float64))
    W = np.abs(ref["W"])
    return (F.sum(1)[:, None] * w_bound(ref) + (ref["d"] + 2) * EPS * (F @ W.T + np.abs(ref["b"])[None, :])
            + b_bound(ref)[None, :])


def logit_bound(ref, F, base, alpha):
    """[B, C]: the error of base + alpha g in fp32: alpha g_bound, and three roundings (alpha b, the product, the sum)."""
    g = np.abs(scores(F, ref["W"], ref["b"]))
    ab = 0.0 if base is None else np.abs(base)
    return alpha * g_bound(ref, F) + 3 * EPS * (ab + alpha * (g + np.abs(ref["b"])[None, :]))


def margin_ratio(ref, F, base, alphas):
    """min over rows and cells of (best - second logit) / (the cell's largest logit error bound of that row)."""
    worst = np.inf
    g = scores(F, ref["W"], ref["b"])
    for a in alphas:
        z = a * g if base is None else base + a * g
        top = -np.sort(-z, axis=1)
        gap = top[:, 0] - top[:, 1]
        worst = min(worst, float((gap / logit_bound(ref, F, base, a).max(1)).min()))
    return worst
