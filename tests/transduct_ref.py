"""The transductive rule of include/clipfs.h ("TRANSDUCT") in numpy, for the tests of csrc/transduct.hip:

    knn, init_state, u_affine, u_mahalanobis, z_step, class_stats, variance, variance_sumsq, fit
        the rule with a ``dtype`` argument: float64 is the reference, float32 the restatement that shows what single
        precision alone costs.  ``fit(..., form="mahalanobis")`` runs steps 4.1 and 4.4 in their textbook form (squared
        distances, sum of squared residuals) instead of the affine / moment form the kernels use.
    chunked_topk
        a model of the kNN launch's column chunks and merge: per chunk a top-k list, then a merge in chunk order.
    synthetic
        the generator: class prototypes around one common direction, noisy features, noisier class features, optional
        shots.
    margins
        the decision margins of a case: the gaps that make exact comparisons of indices and labels fair.
"""
import numpy as np

DEFAULTS = dict(logit_scale=100.0, k=3, init_top=8, lam=1.0, shot_weight=1.0, outer=10, inner=5, n_min=1e-6, var_floor=1e-6)


def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def synthetic(N, C, d, noise, sep, text_noise, seed, shots_per_class=0):
    """(F [N, d], T [C, d], y [N], S [M, d] or None, ys [M] or None), float64 unit rows.  A class prototype is the common
    direction plus ``sep`` times its own Gaussian direction; a feature is its class prototype plus ``noise / sqrt(d)``
    Gaussian noise; a class feature is the prototype plus ``text_noise`` times a unit Gaussian direction; shots are drawn
    like features.  Labels are i mod C shuffled, so every class has members."""
    rng = np.random.default_rng(seed)
    common = _unit(rng.standard_normal((1, d)))
    proto = _unit(common + sep * _unit(rng.standard_normal((C, d))))
    y = rng.permutation(np.arange(N) % C)
    F = _unit(proto[y] + noise / np.sqrt(d) * rng.standard_normal((N, d)))
    T = _unit(proto + text_noise * _unit(rng.standard_normal((C, d))))
    S = ys = None
    if shots_per_class:
        ys = np.repeat(np.arange(C), shots_per_class)
        S = _unit(proto[ys] + noise / np.sqrt(d) * rng.standard_normal((len(ys), d)))
    return F, T, y, S, ys


# ------------------------------------------------------------------------------------------------------------ the rule
def log_softmax(x):
    t = x - x.max(axis=1, keepdims=True)
    return t - np.log(np.exp(t).sum(axis=1, keepdims=True))


def softmax(x):
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def topk_desc(values, k, exclude=None):
    """Indices of the k largest entries, ties to the lower index, in that order (a stable argsort of -values)."""
    order = np.argsort(-values, kind="stable")
    if exclude is not None:
        order = order[order != exclude]
    return order[:k]


def knn(F, k):
    """(nbr [N, k] int32, w [N, k]): step 2."""
    A = F @ F.T
    N = len(F)
    nbr = np.stack([topk_desc(A[i], k, exclude=i) for i in range(N)]).astype(np.int32)
    return nbr, np.take_along_axis(A, nbr.astype(np.int64), axis=1)


def chunked_topk(values, k, chunks, exclude=None):
    """The kNN launch's plan on one row of similarities: the columns are cut into ``chunks`` runs of whole 32-tiles, each
    run keeps its own sorted top-k (value descending, index ascending), and the lists are merged in chunk order under the
    same order.  Returns the indices."""
    n = len(values)
    ntiles = (n + 31) // 32
    per = (ntiles + chunks - 1) // chunks
    better = lambda a, b: a[0] > b[0] or (a[0] == b[0] and a[1] < b[1])

    def insert(lst, item):
        for r in range(len(lst)):
            if better(item, lst[r]):
                lst[r], item = item, lst[r]
        return lst

    lists = []
    for c in range(chunks):
        lst = [(-np.inf, 2 ** 31 - 1)] * k
        for j in range(min(n, c * per * 32), min(n, (c + 1) * per * 32)):
            if j != exclude:
                lst = insert(lst, (values[j], j))
        lists.append(lst)
    out = [(-np.inf, 2 ** 31 - 1)] * k
    for lst in lists:
        for item in lst:
            if item[1] < n:
                out = insert(out, item)
    return np.array([j for _, j in out], dtype=np.int64)


def shot_constants(S, ys, C, d, gamma, dtype):
    """(gamma M_c [C], gamma sum of a class's shots [C, d], gamma sum_j s_jd^2 [d], M)."""
    sn, sG, sq, M = np.zeros(C, dtype), np.zeros((C, d), dtype), np.zeros(d, dtype), 0
    if S is not None and len(S):
        S = S.astype(dtype)
        M = len(S)
        for j, c in enumerate(ys):
            sn[c] += 1
            sG[c] += S[j]
        sn, sG, sq = dtype(gamma) * sn, dtype(gamma) * sG, dtype(gamma) * (S * S).sum(axis=0)
    return sn, sG, sq, M


def init_state(F, logy, m, sn, sG):
    """(sel [C, m], mu [C, d]): step 3's seeds and means."""
    C = logy.shape[1]
    sel = np.stack([topk_desc(logy[:, c], m) for c in range(C)])
    mu = (F[sel].sum(axis=1) + sG) / (m + sn)[:, None]
    return sel.astype(np.int32), mu


def u_affine(F, logy, mu, var, lam):
    mup = mu / var
    b = -0.5 * (mu * mup).sum(axis=1)
    return lam * logy + F @ mup.T + b


def u_mahalanobis(F, logy, mu, var, lam):
    """lam logy - 1/2 sum_d (f_d - mu_cd)^2 / var_d: u_affine plus a term that is constant in c."""
    diff = F[:, None, :] - mu[None, :, :]
    return lam * logy - 0.5 * (diff * diff / var).sum(axis=2)


def z_step(u, nbr, w, z):
    return softmax(u + (w[:, :, None] * z[nbr.astype(np.int64)]).sum(axis=1))


def class_stats(F, z, mu, sn, sG, n_min):
    """(n, G, mu'): step 4.3."""
    n = z.sum(axis=0) + sn
    G = z.T @ F + sG
    move = n > n_min
    new = mu.copy()
    new[move] = G[move] / n[move, None]
    return n, G, new


def variance(Q, mu, G, n, denom, floor):
    """Step 4.4, the moment form."""
    return np.maximum(floor, (Q - 2 * (mu * G).sum(axis=0) + (n[:, None] * mu * mu).sum(axis=0)) / denom)


def variance_sumsq(F, z, mu, S, ys, gamma, denom, floor):
    """Step 4.4 as a weighted sum of squared residuals: sum_ic z_ic (f_id - mu_cd)^2 + gamma sum_j (s_jd - mu_{y_j d})^2.
    Equal to the moment form when z's rows sum to one."""
    diff = F[:, None, :] - mu[None, :, :]
    tot = (z[:, :, None] * diff * diff).sum(axis=(0, 1))
    if S is not None and len(S):
        r = S - mu[ys]
        tot = tot + gamma * (r * r).sum(axis=0)
    return np.maximum(floor, tot / denom)


def fit(F, T, S=None, ys=None, dtype=np.float64, form="affine", nbr_w=None, **hyper):
    """Steps 1 to 5.  Returns a dict: z, labels, zs_labels, mu, var, nbr, w, logy, sel, n, G.  ``nbr_w``: a (nbr, w) pair to
    use instead of this precision's own neighbours."""
    h = {**DEFAULTS, **hyper}
    F, T = F.astype(dtype), T.astype(dtype)
    N, d = F.shape
    C = len(T)
    gamma = dtype(h["shot_weight"])
    logy = log_softmax(dtype(h["logit_scale"]) * (F @ T.T))
    zs = logy.argmax(axis=1)
    nbr, w = nbr_w if nbr_w is not None else knn(F, h["k"])
    w = w.astype(dtype)
    sn, sG, sq, M = shot_constants(S, ys, C, d, gamma, dtype)
    Sd = None if S is None else S.astype(dtype)
    Q = (F * F).sum(axis=0) + sq
    denom = dtype(N + float(gamma) * M)
    z = np.exp(logy)
    var = np.full(d, dtype(1) / dtype(d), dtype)
    sel, mu = init_state(F, logy, h["init_top"], sn, sG)
    n = G = None
    for _ in range(h["outer"]):
        u = (u_affine if form == "affine" else u_mahalanobis)(F, logy, mu, var, dtype(h["lam"]))
        for _ in range(h["inner"]):
            z = z_step(u, nbr, w, z)
        n, G, mu = class_stats(F, z, mu, sn, sG, dtype(h["n_min"]))
        if form == "affine":
            var = variance(Q, mu, G, n, denom, dtype(h["var_floor"]))
        else:
            var = variance_sumsq(F, z, mu, Sd, ys, gamma, denom, dtype(h["var_floor"]))
    return dict(z=z, labels=z.argmax(axis=1), zs_labels=zs, mu=mu, var=var, nbr=nbr, w=w, logy=logy, sel=sel, n=n, G=G)


# ------------------------------------------------------------------------------------------------------------- margins
def margins(F, T, S=None, ys=None, **hyper):
    """The decision margins of a case on the fp64 reference: knn_gap (per row the k-th minus the (k + 1)-th similarity to
    another row, the smallest over rows), init_gap (per class the m-th minus the (m + 1)-th logy, the smallest), top_gap
    (the smallest top-1 minus top-2 of the final z), zs_gap (the same of logy, in nats), moved (labels that differ from
    the zero-shot ones), soft (rows whose largest z is below 0.99) and the fit itself."""
    h = {**DEFAULTS, **hyper}
    k, m = h["k"], h["init_top"]
    A = F @ F.T
    np.fill_diagonal(A, -np.inf)
    a = -np.sort(-A, axis=1)
    ref = fit(F, T, S, ys, **hyper)
    ly = -np.sort(-ref["logy"], axis=0)
    zz = -np.sort(-ref["z"], axis=1)
    lz = -np.sort(-ref["logy"], axis=1)
    two = zz.shape[1] > 1
    return dict(knn_gap=float((a[:, k - 1] - a[:, k]).min()) if a.shape[1] > k + 1 else np.inf,
                init_gap=float((ly[m - 1] - ly[m]).min()) if len(ly) > m else np.inf,
                top_gap=float((zz[:, 0] - zz[:, 1]).min()) if two else 1.0,
                zs_gap=float((lz[:, 0] - lz[:, 1]).min()) if two else np.inf,
                moved=int((ref["labels"] != ref["zs_labels"]).sum()), soft=int((zz[:, 0] < 0.99).sum()), ref=ref)
