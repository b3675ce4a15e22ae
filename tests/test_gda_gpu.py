"""The GDA head on the GPU (csrc/gda.hip, ops.gda_*, gda.GDAHead) against the fp64 rule of gda_ref.py on the pinned
geometries of test_gda_cpu.py.  Every case asserts cond(A) <= 10 (and, for the search, its decision margins) on the fp64
reference before the device is touched, so hits must be EXACT; the float bounds are those of gda_ref.py.

Measured on an MI355X (the prints of these tests; the table of DESIGN.md section 30), G0 .. G3: mu within 0.08 .. 0.28
n_c eps, xt within 0.88 .. 1.95 eps of the largest entry (bound 2), tau within 1.8e-10 .. 9.8e-8 relative, W within
8.1e-8 .. 5.0e-7 of max |W| (bounds 1.2e-5 .. 4.2e-4; 7.3e-7 at shrink 0.5, cond 9.8), b within 0.2 % of its bound, the
applied head within 1.4 % of its logit bound at alpha 1e-2 .. 1e2; search hits exact in every cell (G0: 40 40 40 40 40 40
37 34 34 of 40 over 1e-4 .. 1e4)."""
import numpy as np
import pytest
import torch

import gda_ref as R
from poison import FILLS, poisoned, same_bits
from test_gda_cpu import COND_MAX, GEOS, SEARCH_CASES, SHRINK_GEOS, SHRINKS, assert_search_margins, ref_case

pytestmark = pytest.mark.gpu
EPS = R.EPS


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _dev(x, dev, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).to(dev)


def _np(t):
    return t.double().cpu().numpy() if t.dtype.is_floating_point else t.cpu().numpy()


def _inputs(geo, dev):
    host = torch.from_numpy(geo["offsets"].copy())
    return _dev(geo["S"], dev), host.to(dev), host


def _check_fit(out, geo, ref, tag):
    """The issue's stage bounds on the outputs of a fit (or of the stages)."""
    M, d = geo["M"], geo["d"]
    assert int(out["info"].item()) == 0
    e_mu = (np.abs(_np(out["mu"]) - ref["mu"]) / geo["counts"][:, None]).max()
    xt = _np(out["xt"])
    e_xt = np.abs(xt - ref["xt"]).max() / np.abs(ref["xt"]).max()
    e_tau = abs(float(out["tau"].item()) - ref["tau"]) / ref["tau"]
    e_W = np.abs(_np(out["W"]) - ref["W"]).max()
    e_b = (np.abs(_np(out["b"]) - ref["b"]) / R.b_bound(ref)).max()
    print(f"{tag}: mu {e_mu / EPS:.2f} n_c eps | xt {e_xt / EPS:.2f} eps (bound 2) | tau {e_tau:.2e} (bound {(M + d) * EPS:.2e}) | "
          f"W {e_W / np.abs(ref['W']).max():.2e} of max |W| (bound {R.w_bound(ref) / np.abs(ref['W']).max():.2e}, cond "
          f"{ref['cond']:.2f}) | b {e_b:.3f} of its bound")
    assert e_mu <= EPS
    assert e_xt <= 2 * EPS and not xt[:, M:].any()
    assert e_tau <= (M + d) * EPS
    assert e_W <= R.w_bound(ref)
    assert e_b <= 1.0


def _stages(ops, S, off, host, M, prior, shrink):
    mu, xt = ops.gda_stats(S, off, offsets_host=host)
    gram = ops.gemm_nt(xt, xt, split_k=False)
    gram, tau = ops.gda_shrink(gram, M, shrink)
    chol, info = ops.spd_factor(gram)
    W = ops.spd_solve(chol, mu, alpha=float(S.shape[1]))
    b = ops.gda_bias(mu, W, off, M, prior, offsets_host=host)
    return dict(mu=mu, xt=xt, gram=gram, tau=tau, chol=chol, info=info, W=W, b=b)


@pytest.mark.parametrize("prior", ["uniform", "empirical"])
@pytest.mark.parametrize("name", GEOS)
def test_stages_and_fit(dev, name, prior):
    from clipfs import ops
    geo, ref = ref_case(name, 1.0, prior)
    assert ref["cond"] <= COND_MAX
    S, off, host = _inputs(geo, dev)
    staged = _stages(ops, S, off, host, geo["M"], prior, 1.0)
    runs = []
    for fill in FILLS:
        with poisoned(fill):
            runs.append(ops.gda_fit(S, off, prior=prior, offsets_host=host))
    nohost = ops.gda_fit(S, off, prior=prior)
    torch.cuda.synchronize()
    _check_fit(staged, geo, ref, f"{name} {prior} stages")
    _check_fit(runs[0], geo, ref, f"{name} {prior} fit")
    for other in runs[1:] + [nohost, staged]:  # poisoned outputs, the device offsets alone, the stages one by one
        for key, t in runs[0].items():
            assert same_bits(other[key], t), key
    chol = _np(runs[0]["chol"])
    assert np.array_equal(chol, chol.T) and np.isfinite(chol).all()
    A = _np(runs[0]["gram"])
    assert np.abs(np.tril(chol) @ np.tril(chol).T - A).max() <= 2 * (geo["d"] + 1) * EPS * np.abs(np.diag(A)).max()


@pytest.mark.parametrize("shrink", SHRINKS)
@pytest.mark.parametrize("name", SHRINK_GEOS)
def test_shrink(dev, name, shrink):
    from clipfs import ops
    geo, ref = ref_case(name, shrink)
    assert ref["cond"] <= COND_MAX
    S, off, host = _inputs(geo, dev)
    out = ops.gda_fit(S, off, shrink=shrink, offsets_host=host)
    torch.cuda.synchronize()
    _check_fit(out, geo, ref, f"{name} shrink {shrink}")
    ridge = np.diag(_np(out["gram"])) - np.diag(ref["G"])
    assert np.abs(ridge - shrink * ref["tau"] / (geo["M"] - 1)).max() <= (geo["M"] + geo["d"]) * EPS * np.diag(ref["A"]).max()


@pytest.mark.parametrize("name", GEOS)
def test_head_applies_within_its_bound_and_round_trips(dev, name):
    import gda
    geo, ref = ref_case(name)
    assert ref["cond"] <= COND_MAX
    F, target, base = R.eval_set(geo, 37, 7)
    head = gda.GDAHead.from_features(_dev(geo["S"], dev), _dev(geo["labels"], dev, torch.int64), geo["C"])
    assert head.factor_info() == 0 and head.n_classes == geo["C"]
    assert np.array_equal(_np(head.offsets), geo["offsets"])
    Fd, based = _dev(F, dev), _dev(base, dev)
    for alpha in (1e-2, 1.0, 1e2):
        head.alpha = alpha
        a32 = float(np.float32(alpha))
        for b_np, b_dev in ((base, based), (None, None)):
            got = _np(head(Fd, b_dev))
            want = R.logits(F, ref["W"], ref["b"], b_np, a32)
            ratio = (np.abs(got - want) / R.logit_bound(ref, F, b_np, a32)).max()
            print(f"head {name} alpha {alpha:g} base {b_np is not None}: {ratio:.3f} of the logit bound")
            assert ratio <= 1.0
    # the classes' blocks in reverse order: the stable class sort gives the same head bit for bit
    perm = np.concatenate([np.flatnonzero(geo["labels"] == c) for c in reversed(range(geo["C"]))])
    other = gda.GDAHead.from_features(_dev(geo["S"][perm], dev), _dev(geo["labels"][perm], dev, torch.int64), geo["C"])
    assert same_bits(other.W, head.W) and same_bits(other.b, head.b)
    head.alpha = 0.25
    sd = head.state_dict()
    blank = gda.GDAHead(torch.zeros_like(head.W), torch.zeros_like(head.b), torch.zeros_like(head.mu), torch.zeros_like(head.offsets),
                        torch.ones_like(head.info), prior="empirical", shrink=3.0).to(dev)
    blank.load_state_dict(sd)
    assert (blank.alpha, blank.prior, blank.shrink) == (0.25, "uniform", 1.0) and blank.factor_info() == 0
    assert same_bits(blank(Fd, based), head(Fd, based))
    with pytest.raises(ValueError, match="class 1 has no shot"):
        lab = geo["labels"].copy()
        lab[lab == 1] = 0
        gda.GDAHead.from_features(_dev(geo["S"], dev), _dev(lab, dev, torch.int64), geo["C"])
    with pytest.raises(ValueError, match="no CPU path"):
        head(Fd.cpu())


@pytest.mark.parametrize("name,B,seed", SEARCH_CASES)
def test_search_alpha_hits_are_exact(dev, name, B, seed):
    import gda
    from clipfs import ops
    geo, ref, F, target, base = assert_search_margins(name, B, seed)  # on fp64, before the device is touched
    assert ref["cond"] <= COND_MAX
    g64 = R.scores(F, ref["W"], ref["b"])
    want = R.hits(g64, base, R.DEFAULT_ALPHAS, target)
    head = gda.GDAHead.from_features(_dev(geo["S"], dev), _dev(geo["labels"], dev, torch.int64), geo["C"])
    Fd, based, tgt = _dev(F, dev), _dev(base, dev), _dev(target, dev, torch.int64)
    runs = []
    for fill in FILLS:
        with poisoned(fill):
            runs.append(gda.search_alpha(head, Fd, based, tgt))
    alpha, hits = runs[0]
    print(f"search {name}: hits {_np(hits).tolist()} alpha {alpha:g}")
    assert np.array_equal(_np(hits), want)
    assert alpha == float(np.float32(R.DEFAULT_ALPHAS[int(np.argmax(want))])) == head.alpha  # the first maximum
    for a2, h2 in runs[1:]:
        assert a2 == alpha and same_bits(h2, hits)
    # a caller's grid, a column slice as the base, and no base at all
    grid = (0.5, 2.0, 8.0)
    assert R.margin_ratio(ref, F, base, grid) >= 64 and R.margin_ratio(ref, F, None, grid) >= 64
    wide = torch.full((B, geo["C"] + 3), float("nan"), device=dev)
    wide[:, :geo["C"]] = based
    _a, h = gda.search_alpha(head, Fd, wide[:, :geo["C"]], tgt, alphas=grid)
    assert np.array_equal(_np(h), R.hits(g64, base, grid, target))
    _a, h = gda.search_alpha(head, Fd, None, tgt, alphas=grid)
    assert np.array_equal(_np(h), R.hits(g64, None, grid, target))
    ev = gda.evaluate_gda(head, Fd, based, tgt)
    assert ev["n"] == B and ev["zero_shot"] == (np.argmax(base, 1) == target).mean()


def test_search_ties_go_to_the_lower_class(dev):
    """Two classes tied bit for bit in every cell (equal columns of g and of the base): the lower index must win, in the
    search and in nothing else (the head itself returns logits, not labels)."""
    from clipfs import ops
    B, Cn = 70, 133  # more than one wave pass over the classes, more than one workgroup of rows
    rng = np.random.default_rng(11)
    g = rng.standard_normal((B, Cn)).astype(np.float32)
    base = rng.standard_normal((B, Cn)).astype(np.float32)
    lo, hi = 5, 100  # in different 64-class passes of a lane
    g[:, [lo, hi]] = 9.0
    base[:, [lo, hi]] = 7.0
    g[:35, 70] = 9.0  # a third tied class in between for half the rows
    base[:35, 70] = 7.0
    alphas = torch.tensor([0.5, 1.0, 4.0], device=dev)
    for tgt, want in ((lo, B), (hi, 0), (70, 0)):
        t = torch.full((B,), tgt, device=dev, dtype=torch.int64)
        hits = ops.gda_search(_dev(g, dev), _dev(base, dev), t, alphas)
        assert _np(hits).tolist() == [want] * 3, (tgt, _np(hits))
    hits = ops.gda_search(_dev(g, dev), None, torch.full((B,), lo, device=dev, dtype=torch.int64), alphas)
    assert _np(hits).tolist() == [B] * 3
