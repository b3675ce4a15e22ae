"""The transductive rule without a GPU (tests/transduct_ref.py): the affine form against the Mahalanobis form, the chunked
top-k model against a stable argsort, the margins of the pinned test geometries, fp32 against fp64, and the empty class.

G1 (N 70, C 5, d 64) has soft rows and three row tiles with a ragged last one; G2 (N 150, C 37, d 132) has ragged class
and feature chunks.  Each runs with 0 and with 2 shots per class.  The seeds were found by a search over the first 40; the
conditions asserted below are the contract, not the seed numbers."""
import numpy as np
import pytest

import transduct_ref as R

# name: (N, C, d, noise, separation, class-feature noise, seed)
G1 = (70, 5, 64, 1.5, 0.4, 0.4, 9)
G2 = (150, 37, 132, 1.0, 0.5, 0.5, 37)
GEOS = {"G1": G1, "G2": G2}
CASES = [(g, s) for g in ("G1", "G2") for s in (0, 2)]
CASE_IDS = [f"{g}-{s}shot" for g, s in CASES]

KNN_GAP = 2e-5   # above the worst-case fp32 dot error d 2^-24 of unit rows at both d (7.9e-6 at d = 132)
INIT_GAP = 1e-3  # nats; the fp32 error of logy at s = 100 is s d 2^-24 < 8e-4 in the worst case, ~1e-5 in practice
ZS_GAP = 1e-2    # nats, top-1 minus top-2 of logy: the zero-shot label is compared exactly
TOP_GAP = 0.05   # top-1 minus top-2 of the final z: a z bound of 1e-3 cannot hide a wrong label

_CASE = {}


def case(geo, shots):
    """(F, T, y, S, ys, margins incl. the fp64 fit) of a pinned geometry: computed once, shared, never written."""
    if (geo, shots) not in _CASE:
        N, C, d, noise, sep, tn, seed = GEOS[geo]
        F, T, y, S, ys = R.synthetic(N, C, d, noise, sep, tn, seed, shots)
        _CASE[geo, shots] = (F, T, y, S, ys, R.margins(F, T, S, ys))
    return _CASE[geo, shots]


def assert_margins(geo, shots):
    m = case(geo, shots)[5]
    assert m["knn_gap"] >= KNN_GAP, m["knn_gap"]
    assert m["init_gap"] >= INIT_GAP, m["init_gap"]
    assert m["zs_gap"] >= ZS_GAP, m["zs_gap"]
    assert m["top_gap"] >= TOP_GAP, m["top_gap"]
    assert m["moved"] >= 3, m["moved"]
    if geo == "G1":
        assert m["soft"] >= 3, m["soft"]
    return m


@pytest.mark.parametrize("geo,shots", CASES, ids=CASE_IDS)
def test_pinned_seeds_meet_the_margins(geo, shots):
    m = assert_margins(geo, shots)
    y, ref = case(geo, shots)[2], m["ref"]
    print(f"{geo} {shots} shots: knn gap {m['knn_gap']:.2e}, init gap {m['init_gap']:.2e}, zs gap {m['zs_gap']:.2e}, top gap "
          f"{m['top_gap']:.3f}, moved {m['moved']}, soft {m['soft']}, top-1 {(ref['zs_labels'] == y).mean():.3f} -> "
          f"{(ref['labels'] == y).mean():.3f}")


@pytest.mark.parametrize("geo,shots", CASES, ids=CASE_IDS)
def test_affine_form_equals_mahalanobis_form(geo, shots):
    F, T, _, S, ys, m = case(geo, shots)
    other = R.fit(F, T, S, ys, form="mahalanobis")
    assert np.abs(other["z"] - m["ref"]["z"]).max() <= 1e-10
    assert np.abs(other["mu"] - m["ref"]["mu"]).max() <= 1e-10
    assert np.abs(other["var"] / m["ref"]["var"] - 1).max() <= 1e-10


@pytest.mark.parametrize("geo,shots", CASES, ids=CASE_IDS)
def test_fp32_restatement_is_close_to_fp64(geo, shots):
    F, T, _, S, ys, m = case(geo, shots)
    ref, f32 = m["ref"], R.fit(F, T, S, ys, dtype=np.float32)
    assert f32["z"].dtype == np.float32
    assert np.array_equal(f32["nbr"], ref["nbr"]) and np.array_equal(f32["sel"], ref["sel"])
    assert np.array_equal(f32["labels"], ref["labels"]) and np.array_equal(f32["zs_labels"], ref["zs_labels"])
    ez = np.abs(f32["z"] - ref["z"]).max()
    print(f"{geo} {shots} shots fp32 vs fp64: z {ez:.1e}, mu {np.abs(f32['mu'] - ref['mu']).max():.1e}, var (rel) "
          f"{np.abs(f32['var'] / ref['var'] - 1).max():.1e}")
    assert ez <= 1e-4


@pytest.mark.parametrize("chunks", [1, 2, 3, 4, 5])
def test_chunked_topk_equals_a_stable_argsort(chunks):
    rng = np.random.default_rng(chunks)
    for n, k in ((70, 3), (150, 8), (33, 1), (300, 5)):
        v = rng.standard_normal(n)
        v[rng.integers(0, n, n // 3)] = v[0]  # many exact ties, spread over the chunks
        for exclude in (None, 0, n - 1, n // 2):
            assert np.array_equal(R.chunked_topk(v, k, chunks, exclude), R.topk_desc(v, k, exclude)), (n, k, exclude)
    # a duplicated row: its twin has the same similarity as the row itself and is a legitimate neighbour; self is not
    F = rng.standard_normal((70, 16))
    F /= np.linalg.norm(F, axis=1, keepdims=True)
    F[41] = F[7]
    A = F @ F.T
    for i, twin in ((7, 41), (41, 7)):
        got = R.chunked_topk(A[i], 3, chunks, exclude=i)
        assert got[0] == twin and i not in got
        assert np.array_equal(got, R.knn(F, 3)[0][i])


def test_empty_class_keeps_its_mean_and_everything_stays_finite():
    N, C, d, noise, sep, tn, seed = G1
    F, T, _, _, _ = R.synthetic(N, C, d, noise, sep, tn, seed)
    T = np.concatenate([T, -F.mean(axis=0, keepdims=True) / np.linalg.norm(F.mean(axis=0))])  # points away from all data
    for dtype in (np.float64, np.float32):
        logy = R.log_softmax(dtype(100) * (F.astype(dtype) @ T.astype(dtype).T))
        sn, sG, _, _ = R.shot_constants(None, None, C + 1, d, dtype(1), dtype)
        mu0 = R.init_state(F.astype(dtype), logy, 8, sn, sG)[1]
        out = R.fit(F, T, dtype=dtype)
        assert out["n"][C] <= 1e-6, out["n"][C]  # the class mass underflows ...
        assert np.array_equal(out["mu"][C], mu0[C])  # ... and its mean never moved
        for name in ("z", "mu", "var", "n", "G"):
            assert np.isfinite(out[name]).all(), name
        assert (out["labels"] != C).all()
