"""The kernel ridge head on the GPU (csrc/krr.hip, ops.krr_*, proker.ProKeRHead) against the fp64 rule of krr_ref.py.
Every accuracy case asserts its condition cap on the fp64 reference first; the float bounds are those of krr_ref.py, derived
from the precision and the shapes.  The measured fractions are in the table of DESIGN.md section 32."""
import numpy as np
import pytest
import torch

import krr_ref as R
from poison import FILLS, poisoned, same_bits
from test_krr_cpu import ref_case

pytestmark = pytest.mark.gpu
EPS = R.EPS
GUARD = -777.25
SEARCH = dict(shape=(132, 64, 37), pool=800, B=320, betas=(4.0, 8.0, 20.0), lams=(2.0, 0.5), noise=3.5, scale=0.05, min_ratio=4.0)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _dev(x, dev, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).to(dev)


def _np(t):
    return t.double().cpu().numpy() if t.dtype.is_floating_point else t.cpu().numpy()


def _slice(x, extra, dev):
    """x as a column slice of a wider GUARD-filled buffer: (buffer, view)."""
    buf = torch.full((x.shape[0], x.shape[1] + extra), GUARD, device=dev, dtype=torch.float32)
    buf[:, :x.shape[1]] = x
    return buf, buf[:, :x.shape[1]]


def _ratio(got, want, bound):
    """max |got - want| / bound over the elements with a positive bound; the others must be equal."""
    err = np.abs(got - want)
    assert not err[bound == 0].any()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


# ------------------------------------------------------------------------------------------------ system and targets
@pytest.mark.parametrize("with_base", [False, True])
@pytest.mark.parametrize("n,d,C", [(37, 64, 5), (130, 132, 37)])
def test_system_and_targets(dev, n, d, C, with_base):
    from clipfs import ops
    geo = R.shots(n, d, C)
    n4 = R.n4_of(n)
    assert n4 > n and not np.array_equal(geo["labels"], np.sort(geo["labels"]))
    base_S = R.base_of(geo, geo["S"]) if with_base else None
    ref = R.fit(geo["S"], geo["labels"], C, base_S, 5.5, 0.1, 2.0)
    assert ref["cond"] <= R.COND_CAPS[1]
    S, lab = _dev(geo["S"], dev), _dev(geo["labels"], dev, torch.int32)
    runs = []
    for fill in FILLS:
        with poisoned(fill):
            bbuf, bview = _slice(_dev(base_S, dev), 3, dev) if with_base else (None, None)
            runs.append((ops.krr_system(S, 5.5, 0.1), ops.krr_targets(lab, C, bview, 2.0, labels_host=lab.cpu())))
    torch.cuda.synchronize()
    A, Et = _np(runs[0][0]), _np(runs[0][1])
    low = np.tril_indices(n4)
    r_sys = _ratio(A[low], ref["A"][low], R.system_bound(ref)[low])
    r_tgt = _ratio(Et, ref["Et"], R.targets_bound(ref, base_S))
    print(f"system n {n} d {d}: {r_sys:.3f} of its bound | targets C {C} base {with_base}: {r_tgt:.3f} of its bound")
    assert r_sys <= 1.0 and r_tgt <= 1.0
    assert np.array_equal(A[n:, :], np.eye(n4)[n:, :]) and np.array_equal(A[:, n:], np.eye(n4)[:, n:])  # the pad, exactly
    assert not Et[:, n:].any()
    for a, e in runs[1:]:
        assert same_bits(a, runs[0][0]) and same_bits(e, runs[0][1])
    if with_base:
        assert bool((bbuf[:, C:] == GUARD).all())


# ------------------------------------------------------------------------------------------------ apply
def _apply_case(dev, B, n, C, d, beta=5.5):
    from clipfs import ops
    geo = R.shots(n, d, min(C, n))
    X, _t, _b = R.queries(geo, B, seed=B)
    rng = np.random.default_rng(31 * n + C + d)
    n4 = R.n4_of(n)
    At = R.f32(rng.standard_normal((C, n4)))
    base = R.f32(rng.standard_normal((B, C)))
    At_dev = At.copy()
    At_dev[:, n:] = np.nan  # the sum runs over j < n whatever the pad holds
    Xd, Sd, Atd = _dev(X, dev), _dev(geo["S"], dev), _dev(At_dev, dev)
    bbuf, bview = _slice(_dev(base, dev), 5, dev)
    outs = {}
    for key, b_np, b_dev in (("none", None, None), ("base", base, bview)):
        want = R.apply(X, geo["S"], At, b_np, beta)
        bound = R.apply_bound(X, geo["S"], At, b_np, beta, d)
        obuf = torch.full((B, C + 7), GUARD, device=dev, dtype=torch.float32)
        got = ops.krr_apply(Xd, Sd, Atd, b_dev, beta, out=obuf[:, 2:2 + C])
        fills = []
        for fill in FILLS:
            with poisoned(fill):
                fills.append(ops.krr_apply(Xd, Sd, Atd, b_dev, beta))
        torch.cuda.synchronize()
        r = _ratio(_np(got), want, bound)
        print(f"apply B {B} n {n} C {C} d {d} base {key}: {r:.4f} of its bound")
        assert r <= 1.0
        assert bool((obuf[:, :2] == GUARD).all()) and bool((obuf[:, 2 + C:] == GUARD).all())
        for f in fills:
            assert same_bits(f, got.contiguous())
        outs[key] = got.contiguous()
    assert bool((bbuf[:, C:] == GUARD).all())
    return Xd, Sd, Atd, bview, outs


@pytest.mark.parametrize("d", [64, 132, 512])
@pytest.mark.parametrize("C", [3, 37, 130])
@pytest.mark.parametrize("n", [37, 132])
@pytest.mark.parametrize("B", [1, 33, 70])
def test_apply(dev, B, n, C, d):
    from clipfs import ops
    Xd, Sd, Atd, bview, outs = _apply_case(dev, B, n, C, d)
    if B == 70:  # a row's result depends on neither B nor the other rows
        for b in (0, 33, 69):
            one = ops.krr_apply(Xd[b:b + 1].contiguous(), Sd, Atd, bview[b:b + 1], 5.5)
            assert same_bits(one, outs["base"][b:b + 1])


@pytest.mark.parametrize("C,nt,gy", [(128, 1, 1), (129, 2, 1), (257, 4, 1), (513, 8, 1), (1030, 8, 2)])
def test_apply_across_the_class_boundaries_of_the_plan(dev, C, nt, gy):
    from clipfs import ops
    p = ops.krr_plan(37, C, 64, 33)
    assert (p["tiles_per_wave"], p["apply_grid_y"], p["class_chunk"]) == (nt, gy, 128 * nt)
    _apply_case(dev, 33, 37, C, 64)


def test_apply_matches_the_cache_head_on_one_hot_values(dev):
    """Class-sorted shots and At = alpha * onehot: the product is the Tip-Adapter cache head, computed by another kernel
    (other dot-product and summation orders): twice the kernel value's relative error and the (n + 2) eps of the sum."""
    from clipfs import ops
    n, d, C, B, alpha, beta = 132, 64, 37, 70, 3.0, 5.5
    geo = R.shots(n, d, C)
    order = np.argsort(geo["labels"], kind="stable")
    S, labels = geo["S"][order], geo["labels"][order]
    offsets = np.zeros(C + 1, dtype=np.int32)
    offsets[1:] = np.cumsum(np.bincount(labels, minlength=C))
    X, _t, base = R.queries(geo, B, seed=3)
    At = np.zeros((C, n))
    At[labels, np.arange(n)] = alpha
    Xd, Sd = _dev(X, dev), _dev(S, dev)
    got = _np(ops.krr_apply(Xd, Sd, _dev(At, dev), _dev(base, dev), beta))
    other = _np(ops.cache_logits(Xd, Sd, _dev(offsets, dev, torch.int32), _dev(base, dev), alpha, beta))
    mag = R.kernel(X, S, beta) @ At.T
    bound = (2 * R.g_rel(d, beta) + (n + 2) * EPS) * mag + 2 * EPS * np.abs(base)
    r = _ratio(got, other, bound)
    print(f"apply against cache_logits: {r:.4f} of the summation-order bound")
    assert r <= 1.0


# ------------------------------------------------------------------------------------------------ fit
def _stages(ops, S, lab, C, base, beta, lam, t, panel, panelled):
    A = ops.krr_system(S, beta, lam)
    Et = ops.krr_targets(lab, C, base, t)
    if panelled:
        chol, info = ops.spd_factor_panels(A, panel=panel)
        At = ops.spd_solve_panels(chol, Et, panel=panel)
    else:
        chol, info = ops.spd_factor(A)
        At = ops.spd_solve(chol, Et)
    return dict(A=A, chol=chol, info=info, Et=Et, At=At)


def _fit_case(dev, geo, base_S, ref, panel=256):
    from clipfs import ops
    import proker
    n, d, C = ref["n"], ref["d"], ref["C"]
    plan = ops.krr_plan(n, C, d, 1, panel)
    assert plan["panelled"] == int(ref["n4"] > 1024)
    S, lab, based = _dev(geo["S"], dev), _dev(geo["labels"], dev, torch.int32), _dev(base_S, dev)
    staged = _stages(ops, S, lab, C, based, ref["beta"], ref["lam"], ref["t"], panel, plan["panelled"])
    runs = []
    for fill in FILLS:
        with poisoned(fill):
            runs.append(ops.krr_fit(S, lab, C, based, ref["beta"], ref["lam"], ref["t"], panel, labels_host=lab.cpu()))
    torch.cuda.synchronize()
    fit = runs[0]
    assert int(fit["info"].item()) == 0
    for other in runs[1:] + [staged]:  # poisoned outputs; the stages one by one
        for key in ("A", "chol", "info", "Et", "At"):
            assert same_bits(other[key], fit[key]), key
    At = _np(fit["At"])
    r_at = np.abs(At - ref["At"]).max() / R.at_bound(ref)
    assert not At[:, n:].any()
    # the exact identity, independent of the reference's solver: k(S, S) At^T = Et^T - lambda At^T
    lhs = _np(ops.krr_apply(S, S, fit["At"], based, ref["beta"])) - base_S
    Etd = _np(fit["Et"])
    rhs = (Etd - ref["lam"] * At)[:, :n].T
    id_bound = (R.residual_bound(ref["A"], At, Etd) + 2 * R.g_rel(d, ref["beta"]) * (R.kernel(geo["S"], geo["S"], ref["beta"]) @ np.abs(At[:, :n]).T)
                + R.apply_bound(geo["S"], geo["S"], At, base_S, ref["beta"], d) + 2 * EPS * (np.abs(base_S) + np.abs(rhs)))
    r_id = float((np.abs(lhs - rhs) / id_bound).max())
    # the head's logits
    X, _t, base = R.queries(geo, 70, seed=5)
    head = proker.ProKeRHead.from_features(S, _dev(geo["labels"], dev, torch.int64), C, based, ref["beta"], ref["lam"], ref["t"], panel)
    assert head.factor_info() == 0 and head.n_classes == C and same_bits(head.At, fit["At"])
    got = _np(head(_dev(X, dev), _dev(base, dev)))
    want = R.apply(X, geo["S"], ref["At"], base, ref["beta"])
    r_log = float((np.abs(got - want) / R.logit_bound(ref, X, geo["S"], base)).max())
    print(f"fit n {n} d {d} C {C} beta {ref['beta']:g} lambda {ref['lam']:g} (cond {ref['cond']:.1f}, panelled {plan['panelled']}): "
          f"At {r_at:.4f} | identity {r_id:.4f} | logits {r_log:.4f} of their bounds")
    assert r_at <= 1.0 and r_id <= 1.0 and r_log <= 1.0
    return head


@pytest.mark.parametrize("k", range(len(R.SETTINGS)))
@pytest.mark.parametrize("shape", R.SHAPES)
def test_fit_and_head(dev, shape, k):
    geo, base_S, ref = ref_case(shape, k)
    assert ref["cond"] <= R.COND_CAPS[k]  # a case that misses its cap is a bad input, not a loose tolerance
    _fit_case(dev, geo, base_S, ref)


def test_the_largest_system_of_the_fused_route(dev):
    """n4 = 1024 is the last size of ops.spd_factor / ops.spd_solve (n = 1022 also pads); test_fit_and_head's n = 1028 is
    the first of the panelled pair.  Both routes are asserted on the plan inside _fit_case."""
    from clipfs import ops
    assert ops.krr_plan(1022, 64, 128)["panelled"] == 0 and ops.krr_plan(1028, 64, 128)["panelled"] == 1
    geo = R.shots(1022, 128, 64)
    base_S = R.base_of(geo, geo["S"])
    ref = R.fit(geo["S"], geo["labels"], 64, base_S, *R.SETTINGS[0])
    assert ref["n4"] == 1024 and ref["cond"] <= R.COND_CAPS[0]
    _fit_case(dev, geo, base_S, ref)


# ------------------------------------------------------------------------------------------------ head
def search_reference():
    """The fp64 side of the search case: (geo, base_S, X, base, target, hits [nB, nL], min margin ratio).  The validation
    rows are the first SEARCH["B"] of SEARCH["pool"] seeded candidates whose top-1 margin is at least min_ratio times twice
    their logit bound in EVERY cell: rows whose decision no fp32 error within the bounds can flip, chosen on fp64 alone."""
    n, d, C = SEARCH["shape"]
    geo = R.shots(n, d, C)
    base_S = R.base_of(geo, geo["S"], scale=SEARCH["scale"])
    X, target, base = R.queries(geo, SEARCH["pool"], seed=10, noise=SEARCH["noise"], scale=SEARCH["scale"])
    cells, ratio = {}, np.full(SEARCH["pool"], np.inf)
    for beta in SEARCH["betas"]:
        for lam in SEARCH["lams"]:
            ref = R.fit(geo["S"], geo["labels"], C, base_S, beta, lam)
            assert ref["cond"] <= 25.0
            z = R.apply(X, geo["S"], ref["At"], base, beta)
            top = -np.sort(-z, axis=1)
            ratio = np.minimum(ratio, (top[:, 0] - top[:, 1]) / (2 * R.logit_bound(ref, X, geo["S"], base).max(1)))
            cells[(beta, lam)] = z
    rows = np.flatnonzero(ratio >= SEARCH["min_ratio"])[:SEARCH["B"]]
    assert rows.size == SEARCH["B"]
    hits = np.array([[R.hits(cells[(b, l)][rows], target[rows]) for l in SEARCH["lams"]] for b in SEARCH["betas"]])
    return geo, base_S, X[rows], base[rows], target[rows], hits, float(ratio[rows].min())


def test_head_round_trip_and_search(dev):
    import proker
    geo, base_S, X, base, target, want, worst = search_reference()  # on fp64, before the device is touched
    flat = np.sort(want.ravel())
    assert worst >= SEARCH["min_ratio"] and flat[-1] - flat[-2] >= 1, (worst, want)  # exact hits, a unique best cell
    n, d, C = SEARCH["shape"]
    S, lab, based = _dev(geo["S"], dev), _dev(geo["labels"], dev, torch.int64), _dev(base_S, dev)
    Xd, bd, tgt = _dev(X, dev), _dev(base, dev), _dev(target, dev, torch.int64)
    beta, lam, hits = proker.search_hp(S, lab, C, based, Xd, bd, tgt, SEARCH["betas"], SEARCH["lams"])
    print(f"search_hp: hits {_np(hits).tolist()} -> beta {beta:g} lambda {lam:g} (margin ratio {worst:.1f})")
    assert np.array_equal(_np(hits), want)
    bi, li = np.unravel_index(int(np.argmax(want)), want.shape)
    assert (beta, lam) == (SEARCH["betas"][bi], SEARCH["lams"][li])
    head = proker.ProKeRHead.from_features(S, lab, C, based, beta, lam, 1.0, 128)
    sd = head.state_dict()
    blank = proker.ProKeRHead(torch.zeros_like(head.shots), torch.zeros_like(head.At), torch.ones_like(head.info), beta=9.0, lam=3.0,
                              target_scale=2.0, panel=64).to(dev)
    blank.load_state_dict(sd)
    assert (blank.beta, blank.lam, blank.target_scale, blank.panel) == (beta, lam, 1.0, 128) and blank.factor_info() == 0
    assert same_bits(blank.At, head.At) and same_bits(blank.shots, head.shots)
    assert same_bits(blank(Xd, bd), head(Xd, bd))
    with pytest.raises(ValueError, match="no CPU path"):
        head(Xd.cpu())
    with pytest.raises(ValueError, match="labels outside"):
        proker.ProKeRHead.from_features(S, lab + 1, C)
