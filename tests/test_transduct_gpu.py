"""Transductive inference on the GPU (csrc/transduct.hip, ops.transduct_*, transclip.TransductiveClassifier) against the fp64
rule of transduct_ref.py, on the pinned geometries of test_transduct_cpu.py.  Every case asserts its decision margins on
the fp64 reference before the device is touched, so neighbour indices, seed rows and labels must be EXACT; the float
bounds are the issue's.

Measured on an MI355X (the prints of these tests; the table of DESIGN.md section 29): kNN weights within 1.2e-7 of fp64,
one z sweep within 3.9e-7 / 1.2e-6 / 9.0e-7 / 4.1e-7 at C 5 / 37 / 300 / 1030 (bound 1e-4), statistics within 1.6e-7 of
the largest entry and 2.9e-7 relative in the variance, the fit within 4.3e-6 in z, 8.7e-8 in mu and 3.5e-7 relative in
the variance."""
import numpy as np
import pytest
import torch

import transduct_ref as R
from poison import FILLS, FILL_IDS, same_bits
from test_transduct_cpu import CASE_IDS, CASES, GEOS, KNN_GAP, assert_margins, case

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _dev(x, dev, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).to(dev)


def _np(t):
    return t.double().cpu().numpy() if t.dtype.is_floating_point else t.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------- 1. kNN
KNN_SEED = 8  # of the N 300, d 132 case: the smallest gap at k = 1, 3 and 8 is asserted below
_KNN = {}


def _knn_case(name):
    """(F fp64, {k: (nbr, w)}) for 'G1', 'G2' or 'N300': computed once, shared, never written."""
    if name not in _KNN:
        if name == "N300":
            F = R.synthetic(300, 37, 132, 1.0, 0.5, 0.5, KNN_SEED)[0]
            ks = (1, 3, 8)
        else:
            F = case(name, 0)[0]
            ks = (3,)
        A = F @ F.T
        np.fill_diagonal(A, -np.inf)
        a = -np.sort(-A, axis=1)
        for k in ks:
            assert (a[:, k - 1] - a[:, k]).min() >= KNN_GAP, (name, k, (a[:, k - 1] - a[:, k]).min())
        _KNN[name] = (F, {k: R.knn(F, k) for k in ks})
    return _KNN[name]


@pytest.mark.parametrize("name,k", [("G1", 3), ("G2", 3), ("N300", 1), ("N300", 3), ("N300", 8)])
def test_knn(dev, name, k):
    from clipfs import ops
    F, want = _knn_case(name)
    nbr_w, w_w = want[k]
    F32 = _dev(F, dev)
    d = F.shape[1]
    runs = [ops.transduct_knn(F32, k, knn_chunks=c) for c in (1, 2, 5, 0, 1)]
    torch.cuda.synchronize()
    nbr, w = runs[0]
    assert np.array_equal(_np(nbr), nbr_w)  # sets and order
    err = np.abs(_np(w) - w_w).max()
    print(f"knn {name} k {k}: max |w - fp64| = {err:.2e} (bound {2 * d * EPS:.2e})")
    assert err <= 2 * d * EPS
    for other_nbr, other_w in runs[1:]:  # across chunk counts and across two runs
        assert same_bits(other_nbr, nbr) and same_bits(other_w, w)


def test_knn_duplicated_row_finds_its_twin_not_itself(dev):
    from clipfs import ops
    F = case("G1", 0)[0].astype(np.float32).copy()
    F[41] = F[7]
    F32 = torch.from_numpy(F).to(dev)
    for chunks in (1, 2, 3):
        nbr, w = ops.transduct_knn(F32, 3, knn_chunks=chunks)
        nbr, w = _np(nbr), _np(w)
        assert nbr[7, 0] == 41 and nbr[41, 0] == 7
        assert (nbr != np.arange(70)[:, None]).all()
        assert w[7, 0] == w[41, 0] and abs(w[7, 0] - 1) < 1e-5
        assert (np.diff(w, axis=1) <= 0).all()


# ------------------------------------------------------------------------------------------------- 2. logy and init
@pytest.mark.parametrize("geo,shots", CASES, ids=CASE_IDS)
def test_logy_and_init(dev, geo, shots):
    from clipfs import ops
    F, T, _, S, ys, _ = case(geo, shots)
    ref = assert_margins(geo, shots)["ref"]
    d = F.shape[1]
    F32, T32 = _dev(F, dev), _dev(T, dev)
    logy, zs, z0 = ops.transduct_logy(F32, T32)
    assert np.array_equal(_np(zs), ref["zs_labels"])
    el = np.abs(_np(logy) - ref["logy"]).max()
    # a logit is s times a dot of unit rows (error <= 2 d 2^-24 s), the log-sum-exp adds a few ulps of |logy| <~ 100
    bound = 100 * 2 * d * EPS + 100 * 8 * EPS
    print(f"logy {geo}: max |logy - fp64| = {el:.2e} (bound {bound:.2e})")
    assert el <= bound
    assert np.abs(_np(z0) - np.exp(ref["logy"])).max() <= 2 * bound  # |d exp| <= |d logy| for logy <= 0
    S32 = None if S is None else _dev(S, dev)
    y32 = None if ys is None else torch.from_numpy(ys).int()
    out = ops.transduct_init(F32, logy, S32, y32)
    assert np.array_equal(_np(out["sel"]), ref["sel"])  # the seed rows, in rank order
    gamma = 1.0
    sn, sG, sq, M = R.shot_constants(S, ys, len(T), d, gamma, np.float64)
    mu0 = R.init_state(F, ref["logy"], 8, sn, sG)[1]
    em = np.abs(_np(out["mu"]) - mu0).max()
    print(f"init {geo} {shots} shots: max |mu - fp64| = {em:.2e}")
    assert em <= 1e-6
    assert np.abs(_np(out["var"]) - 1 / d).max() <= 1e-8 and np.abs(_np(out["mup"]) - mu0 * d).max() <= 1e-6 * d
    assert np.abs(_np(out["shot_n"]) - sn).max() == 0 and np.abs(_np(out["shot_G"]) - sG).max() <= 1e-6
    assert np.abs(_np(out["Q"]) - ((F * F).sum(axis=0) + sq)).max() <= 1e-5 * ((F * F).sum(axis=0) + sq).max()


# ----------------------------------------------------------------------------------------------------- 3. one z sweep
@pytest.mark.parametrize("C", [5, 37, 300, 1030])  # 300 and 1030 cross the 256- and 1024-class register chunks
def test_z_step(dev, C):
    from clipfs import ops
    rng = np.random.default_rng(C)
    N, k = 70, 3
    z = R.softmax(3 * rng.standard_normal((N, C)))
    u = rng.uniform(-50, 50, (N, C))
    nbr = rng.integers(0, N, (N, k)).astype(np.int32)
    w = rng.uniform(0, 1, (N, k))
    u32, z32, w32 = _dev(u, dev), _dev(z, dev), _dev(w, dev)
    want = R.z_step(_np(u32), nbr, _np(w32), _np(z32))  # fp64 arithmetic on the fp32 inputs the kernel reads
    got, labels = ops.transduct_z_step(u32, torch.from_numpy(nbr).to(dev), w32, z32, want_labels=True)
    again = ops.transduct_z_step(u32, torch.from_numpy(nbr).to(dev), w32, z32)
    err = np.abs(_np(got) - want).max()
    print(f"z_step C {C}: max |z - fp64| = {err:.2e}")
    assert err <= 1e-4
    assert same_bits(got, again)
    assert np.abs(_np(got).sum(axis=1) - 1).max() <= 1e-5
    srt = -np.sort(-want, axis=1)
    clear = (srt[:, 0] - srt[:, 1]) > 1e-3
    assert clear.sum() >= 10 and np.array_equal(_np(labels)[clear], want.argmax(axis=1)[clear])
    assert np.array_equal(_np(labels), _np(got).argmax(axis=1))  # ties low, on the stored values


# --------------------------------------------------------------------------------------------------- 4. class statistics
@pytest.mark.parametrize("shots", [0, 2])
@pytest.mark.parametrize("geo", ["G1", "G2"])
def test_stats(dev, geo, shots):
    from clipfs import ops
    F, T, _, S, ys, _ = case(geo, shots)
    (N, d), C = F.shape, len(T)
    rng = np.random.default_rng(5)
    z = R.softmax(3 * rng.standard_normal((N, C)))
    z[:, 1] = 0.0  # an empty class: without shots n_1 = 0 <= n_min and its mean stays
    mu_in = rng.standard_normal((C, d)) / np.sqrt(d)
    F32, z32, mu32 = _dev(F, dev), _dev(z, dev), _dev(mu_in, dev)
    Fd, zd, mud = _np(F32), _np(z32), _np(mu32)
    Sd = None if S is None else _np(_dev(S, dev))
    sn, sG, sq, M = R.shot_constants(Sd, ys, C, d, 1.0, np.float64)
    Q = (Fd * Fd).sum(axis=0) + sq
    n_w, G_w, mu_w = R.class_stats(Fd, zd, mud, sn, sG, 1e-6)
    var_free = R.variance(Q, mu_w, G_w, n_w, N + M, 0.0)
    floor = float(np.median(var_free))  # half of the variances sit on the floor, half above it
    var_w = np.maximum(floor, var_free)
    assert (var_free < floor).sum() >= d // 4 and (var_free > floor).sum() >= d // 4
    if shots == 0:
        assert n_w[1] <= 1e-6 and np.array_equal(mu_w[1], mud[1])
    out = ops.transduct_stats(F32, z32, mu32, _dev(sn, dev), _dev(sG, dev), _dev(Q, dev), M=M, var_floor=floor)
    again = ops.transduct_stats(F32, z32, mu32, _dev(sn, dev), _dev(sG, dev), _dev(Q, dev), M=M, var_floor=floor)
    errs = {k: np.abs(_np(out[k]) - wv).max() / np.abs(wv).max() for k, wv in (("n", n_w), ("G", G_w), ("mu", mu_w))}
    ev = np.abs(_np(out["var"]) / var_w - 1).max()
    print(f"stats {geo} {shots} shots: n {errs['n']:.1e} G {errs['G']:.1e} mu {errs['mu']:.1e} of the largest entry, var "
          f"(rel) {ev:.1e}")
    assert max(errs.values()) <= 1e-5 and ev <= 1e-4
    if shots == 0:
        assert same_bits(out["mu"][1], mu32[1])  # the empty class kept its mean bit for bit
    on_floor = var_free < floor * (1 - 1e-3)
    assert (_np(out["var"])[on_floor] == np.float32(floor)).all()  # the floor branch, exactly
    assert np.abs(_np(out["mup"]) - _np(out["mu"]) / _np(out["var"])).max() <= 1e-6 * np.abs(_np(out["mup"])).max()
    for name in out:
        assert same_bits(out[name], again[name]), name


# ------------------------------------------------------------------------------------------------------ 5. the whole fit
OUTPUTS = ("z", "labels", "zs_labels", "mu", "var", "nbr", "w")


def _inputs(geo, shots, dev):
    F, T, _, S, ys, _ = case(geo, shots)
    return (_dev(F, dev), _dev(T, dev), None if S is None else _dev(S, dev),
            None if ys is None else torch.from_numpy(ys).int())


def _staged(F32, T32, S32, y32, hyper):
    """The fit composed from the stage ops, one call per stage."""
    from clipfs import ops
    M = 0 if S32 is None else S32.shape[0]
    logy, zs, z = ops.transduct_logy(F32, T32)
    nbr, w = ops.transduct_knn(F32, hyper["k"])
    st = ops.transduct_init(F32, logy, S32, y32)
    mu, mup, var = st["mu"], st["mup"], st["var"]
    labels, left = None, hyper["outer"] * hyper["inner"]
    for _ in range(hyper["outer"]):
        u, _ = ops.transduct_u(F32, logy, mu, mup)
        for _ in range(hyper["inner"]):
            left -= 1
            if left == 0:
                z, labels = ops.transduct_z_step(u, nbr, w, z, want_labels=True)
            else:
                z = ops.transduct_z_step(u, nbr, w, z)
        s = ops.transduct_stats(F32, z, mu, st["shot_n"], st["shot_G"], st["Q"], M=M)
        mu, mup, var = s["mu"], s["mup"], s["var"]
    return dict(z=z, labels=labels, zs_labels=zs, mu=mu, var=var, nbr=nbr, w=w)


@pytest.mark.parametrize("geo,shots", CASES, ids=CASE_IDS)
def test_fit(dev, geo, shots):
    from clipfs import ops
    ref = assert_margins(geo, shots)["ref"]
    F32, T32, S32, y32 = _inputs(geo, shots, dev)
    out = ops.transduct_fit(F32, T32, S32, y32)
    assert np.array_equal(_np(out["labels"]), ref["labels"]) and np.array_equal(_np(out["zs_labels"]), ref["zs_labels"])
    assert np.array_equal(_np(out["nbr"]), ref["nbr"]) and np.array_equal(_np(out["sel"]), ref["sel"])
    ez, em = np.abs(_np(out["z"]) - ref["z"]).max(), np.abs(_np(out["mu"]) - ref["mu"]).max()
    ev = np.abs(_np(out["var"]) / ref["var"] - 1).max()
    print(f"fit {geo} {shots} shots: z {ez:.1e}, mu {em:.1e}, var (rel) {ev:.1e}")
    assert ez <= 1e-3 and em <= 1e-5 and ev <= 1e-4
    again = ops.transduct_fit(F32, T32, S32, y32)
    staged = _staged(F32, T32, S32, y32, ops.TRANSDUCT_DEFAULTS)
    forced = ops.transduct_fit(F32, T32, S32, y32, knn_chunks=2)
    for name in OUTPUTS:
        assert same_bits(out[name], again[name]), f"{name}: run to run"
        assert same_bits(out[name], staged[name]), f"{name}: fit against the stages one by one"
        assert same_bits(out[name], forced[name]), f"{name}: forced kNN chunks"


# ------------------------------------------------------------------------------------------------------------ 6. poison
GUARD = 16


@pytest.mark.parametrize("geo,shots", [("G2", 2), ("G1", 0)], ids=["G2-2shot", "G1-0shot"])
def test_fit_does_not_depend_on_what_its_buffers_held(dev, geo, shots):
    """Every output, state and work buffer of the fit is pre-filled with 0 / NaN / 1e30 (integers: 0, they are indices)
    with GUARD more elements behind it.  No output bit changes and every guard keeps its fill."""
    from clipfs import ops
    F32, T32, S32, y32 = _inputs(geo, shots, dev)
    (N, d), C = F32.shape, T32.shape[0]
    M = 0 if S32 is None else S32.shape[0]
    clean = ops.transduct_fit(F32, T32, S32, y32, knn_chunks=2)
    shapes = ops.transduct_shapes(N, C, d, M, knn_chunks=2)
    for fill, fid in zip(FILLS, FILL_IDS):
        big, bufs = {}, {}
        for name, (shape, dt) in shapes.items():
            numel = int(np.prod(shape))
            big[name] = torch.full((numel + GUARD,), fill if dt.is_floating_point else 0, device=dev, dtype=dt)
            if not dt.is_floating_point:
                big[name][numel:] = -7
            bufs[name] = big[name][:numel].view(shape)
        out = ops.transduct_fit(F32, T32, S32, y32, knn_chunks=2, buffers=bufs)
        torch.cuda.synchronize()
        for name in OUTPUTS + ("sel", "n", "G", "mup", "bias", "logy", "u"):
            assert same_bits(out[name], clean[name]), f"{name}: fill {fid}"
            if out[name].dtype.is_floating_point:
                assert torch.isfinite(out[name]).all(), name
        for name, (shape, dt) in shapes.items():
            guard = big[name][int(np.prod(shape)):]
            want = torch.full_like(guard, fill if dt.is_floating_point else -7)
            assert same_bits(guard, want), f"{name}: guard overwritten under fill {fid}"


# -------------------------------------------------------------------------------------------------------- 7. the module
def _torch_route(F, T, hyper):
    """One outer iteration composed from torch: dense F F^T + topk, index gather, softmax, z.T @ F."""
    s, k, m, lam = hyper["logit_scale"], hyper["k"], hyper["init_top"], hyper["lam"]
    N, d = F.shape
    logy = torch.log_softmax(s * (F @ T.T), dim=1)
    A = F @ F.T
    A.fill_diagonal_(float("-inf"))
    w, nbr = torch.topk(A, k, dim=1)
    z = logy.exp()
    var = torch.full((d,), 1.0 / d, device=F.device)
    sel = torch.topk(logy, m, dim=0).indices.T  # [C, m]
    mu = F[sel].sum(dim=1) / m
    mup = mu / var
    u = lam * logy + F @ mup.T - 0.5 * (mu * mup).sum(dim=1)
    for _ in range(hyper["inner"]):
        z = torch.softmax(u + (w[:, :, None] * z[nbr]).sum(dim=1), dim=1)
    n = z.sum(dim=0)
    G = z.T @ F
    mu = torch.where((n > hyper["n_min"])[:, None], G / n[:, None], mu)
    var = ((F * F).sum(dim=0) - 2 * (mu * G).sum(dim=0) + (n[:, None] * mu * mu).sum(dim=0)) / N
    return z, mu, var.clamp_min(hyper["var_floor"]), nbr


@pytest.mark.parametrize("geo", ["G1", "G2"])
def test_classifier_one_outer_iteration_equals_the_torch_route(dev, geo):
    from clipfs import ops
    from transclip import TransductiveClassifier
    assert_margins(geo, 0)
    F32, T32, _, _ = _inputs(geo, 0, dev)
    clf = TransductiveClassifier(T32, outer=1)
    res = clf.fit_predict(F32)
    z, mu, var, nbr = _torch_route(F32, ops.l2norm_fwd(T32), clf.hyper)
    assert torch.equal(res.neighbours.long(), nbr)
    ez, em = (res.z - z).abs().max().item(), (res.mu - mu).abs().max().item()
    ev = (res.var / var - 1).abs().max().item()
    print(f"classifier {geo}, outer 1, against torch: z {ez:.1e}, mu {em:.1e}, var (rel) {ev:.1e}")
    assert ez <= 1e-3 and em <= 1e-5 and ev <= 1e-4
    top = z.topk(2, dim=1).values
    clear = (top[:, 0] - top[:, 1]) > 1e-2  # ten times the z bound
    assert clear.sum().item() >= len(z) // 2 and torch.equal(res.labels.long()[clear], z.argmax(dim=1)[clear])


def test_evaluate_transductive_runs_on_the_tiny_model(dev):
    from clipfs import synth
    from jclip.model import build_model
    from transclip import TransductiveClassifier, evaluate_transductive
    model = build_model(synth.synth_state_dict(synth.TINY, seed=2), device=dev)
    C, n = 6, 24
    prompts = synth.synth_captions(C, synth.TINY.context_length, synth.TINY.vocab_size, seed=4, max_len=10)
    images = synth.synth_images(n, synth.TINY.image_resolution, seed=3).to(dev)
    target = synth.synth_labels(n, C, seed=2)
    clf = TransductiveClassifier(clip_model=model, tokenized_prompts=prompts, n_classes=C, outer=2, inner=2)
    acc = evaluate_transductive(model, [(images[:10], target[:10]), (images[10:], target[10:])], clf)
    assert acc["n"] == n and 0.0 <= acc["top1_zero_shot"] <= 1.0 and 0.0 <= acc["top1_transductive"] <= 1.0
    res = clf.fit_predict_images(images)
    assert torch.isfinite(res.z).all() and (res.z.sum(dim=1) - 1).abs().max().item() <= 1e-5
    with pytest.raises(ValueError, match="alpha"):
        TransductiveClassifier(torch.zeros(3, 8), alpha=1.0)
    with pytest.raises(ValueError, match="k = 9"):
        TransductiveClassifier(torch.zeros(3, 8), k=9)
