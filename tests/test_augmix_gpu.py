"""AugMix views on the device (csrc/augmix.hip + clipfs/augmix.py) against PIL itself (tests/augmix_ref.py): every uint8
image bit for bit, the fp32 view bit for bit against the numpy float32 mix; plain views against data.crop_batch; workspace
independence; the public entry points; the multi-view front end of the TDA adapter.  Every comparison is exact."""
import numpy as np
import pytest
import torch

import augmix_ref as R

pytestmark = pytest.mark.gpu
MAX_CALL = 16  # views per call in these tests


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _sources():
    return [R.image(40, 57, 8), R.image(375, 500, 1)]


def _run(pool, recs, recipe, S, **kw):
    """(out [n, 3, S, S], base_u8 [n, S, S, 3], chains_u8 [n, width, S, S, 3]) as numpy, at most MAX_CALL views a call."""
    from clipfs import augmix as A
    parts = []
    for lo in range(0, len(recs), MAX_CALL):
        sl = slice(lo, lo + MAX_CALL)
        o, b, c = A.augmix_batch(pool, recs[sl], A.Recipe(*(t[sl] for t in recipe)), S, keep_u8=True, **kw)
        parts.append((o.cpu().numpy(), b.cpu().numpy(), c.cpu().numpy()))
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_against_pil(arrays, recs, recipe, S, got, names=None):
    from clipfs.views import CLIP_MEAN, CLIP_STD
    out, base, chains = got
    for v, rec in enumerate(recs):
        tag = (S, v, names[v] if names else tuple(int(x) for x in rec))
        wb, wc, wo = R.pil_view(arrays[rec[0]], rec, recipe, v, S, CLIP_MEAN, CLIP_STD)
        assert np.array_equal(base[v], wb), ("base_u8", tag)
        assert np.array_equal(chains[v], wc), ("chains_u8", tag, recipe.ops[v].tolist(), recipe.depth[v].tolist())
        assert np.array_equal(_bits(out[v]), _bits(wo)), ("out", tag)


# ------------------------------------------------------------------------------------------- 1. each operation alone
@pytest.mark.parametrize("S", [224, 37, 8])
def test_each_operation_alone_equals_pil(dev, S):
    from clipfs import augmix as A
    from clipfs import data, views
    cases = R.edge_cases(S)
    arrays, index = [], {}
    for _, u8, _, _, _ in cases:  # the distinct S x S images are the pool: an S -> S bilinear crop is the image itself
        if id(u8) not in index:
            index[id(u8)] = len(arrays)
            arrays.append(u8)
    pool = data.ImagePool.from_arrays(arrays, list(range(len(arrays))), device=dev)
    n = len(cases)
    recs = np.asarray([(index[id(u8)], 0, 0, S, S, 0, S, S, 0, 0, views.BILINEAR, 0) for _, u8, _, _, _ in cases], np.int32)
    ops = np.zeros((n, 1, 3, 2), np.int32)
    coef = np.tile(np.asarray(A.IDENTITY), (n, 1, 3, 1))
    for v, (_, _, code, param, co) in enumerate(cases):
        ops[v, 0, 0] = (code, param)
        coef[v, 0, 0] = co
    recipe = A.Recipe(ops, coef, np.ones((n, 1), np.int32), np.ones((n, 1), np.float32), np.zeros(n, np.float32))
    got = _run(pool, recs, recipe, S)
    for v, (name, u8, code, param, co) in enumerate(cases):
        assert np.array_equal(got[1][v], u8), (S, name)
        assert np.array_equal(got[2][v, 0], R.pil_op(u8, code, param, co)), (S, name)
    _check_against_pil(arrays, recs, recipe, S, got, [c[0] for c in cases])


# ----------------------------------------------------------------------------------------------- 2. whole recipes
def _mixed_records(arrays, S, n, seed):
    """n records over the sources in turn: random resized crops with flips, and one bicubic centre record per source."""
    from clipfs import views
    rng = np.random.RandomState(seed)
    recs = []
    for v in range(n):
        i = v % len(arrays)
        H, W = arrays[i].shape[:2]
        if v < len(arrays):
            recs.append((i,) + views.centre_view_record(W, H, 256, S) + (0,))
        else:
            # the kernel takes 80 filter taps: a bilinear box side of at most 39 S (S = 8: boxes up to 304 px of the 500)
            hi = min(1.0, 0.75 * (38 * S) ** 2 / (W * H))
            top, left, h, w = views.sample_crop(W, H, (min(0.08, hi), hi), (3 / 4, 4 / 3), rng)
            recs.append((i, top, left, h, w, v % 3 != 0, S, S, 0, 0, views.BILINEAR, 0))
    return np.asarray(recs, np.int32)


def _recipe12(S, seed=4):
    from clipfs import augmix as A
    r = A.sample_recipes(12, S, width=3, severity=3, seed=seed)
    # two AFFINE steps in a row, and EQUALIZE / AUTOCONTRAST after AFFINE (the histogram must see the fill)
    r.depth[0, 0], r.depth[1, 1], r.depth[2, 2] = 2, 2, 3
    r.ops[0, 0, :2] = [(A.AFFINE, 0), (A.AFFINE, 0)]
    r.coef[0, 0, 0], r.coef[0, 0, 1] = A.rotate_coefficients(-9, S), (1.0, 0.09, 0.0, 0.0, 1.0, 0.0)
    r.ops[1, 1, :2] = [(A.AFFINE, 0), (A.EQUALIZE, 0)]
    r.coef[1, 1, 0] = (1.0, 0.0, float(S // 4), 0.0, 1.0, 0.0)
    r.ops[2, 2] = [(A.POSTERIZE, 3), (A.AFFINE, 0), (A.AUTOCONTRAST, 0)]
    r.coef[2, 2, 1] = (1.0, 0.0, 0.0, -0.07, 1.0, 1.5)
    return r


@pytest.mark.parametrize("S", [224, 37, 8])
def test_whole_recipes_equal_pil(dev, S):
    from clipfs import data
    arrays = _sources()
    pool = data.ImagePool.from_arrays(arrays, [0, 1], device=dev)
    recs = _mixed_records(arrays, S, 12, seed=S)
    recipe = _recipe12(S)
    assert recs[:, 5].any() and (recs[:, 10] == 1).sum() == 2 and set(recipe.ops[..., 0].reshape(-1)) >= {1, 2, 3, 4, 5}
    _check_against_pil(arrays, recs, recipe, S, _run(pool, recs, recipe, S))


# ------------------------------------------------------------------------------------------------- 3. plain views
@pytest.mark.parametrize("S", [224, 37])
def test_plain_views_are_crop_batch(dev, S):
    from clipfs import augmix as A
    from clipfs import data
    arrays = _sources()
    pool = data.ImagePool.from_arrays(arrays, [0, 1], device=dev)
    recs = _mixed_records(arrays, S, 8, seed=11)
    recipe = A.sample_recipes(8, S, width=3, severity=3, seed=2, plain=np.ones(8, bool))
    out, base, chains = _run(pool, recs, recipe, S)
    norm = torch.empty(8, 3, S, S, device=dev)
    raw = torch.empty(8, 3, S, S, device=dev)
    data.crop_batch(pool, recs, S, norm, raw)
    assert np.array_equal(_bits(out), _bits(norm.cpu().numpy()))
    assert np.array_equal(_bits(base.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255)), _bits(raw.cpu().numpy()))
    for i in range(3):
        assert np.array_equal(chains[:, i], base)  # a chain of depth 0 is base itself


# ------------------------------------------------------------------------------- 4. workspace and independence
def test_workspace_independence_repeat_slices_and_streams(dev):
    from clipfs import augmix as A
    from clipfs import data
    S, n = 37, 12
    arrays = _sources()
    pool = data.ImagePool.from_arrays(arrays, [0, 1], device=dev)
    recs = _mixed_records(arrays, S, n, seed=5)
    recipe = _recipe12(S, seed=6)
    base_c, chains_c = A._u8_buffers(dev, n, 3, S, False)  # the cached pair the calls below reuse
    runs = []
    for fill_u8, fill_out in ((0x00, 0.0), (0xFF, float("nan")), (0x5A, 1.0e30)):
        base_c.fill_(fill_u8)
        chains_c.fill_(fill_u8)
        out = torch.full((n, 3, S, S), fill_out, device=dev)
        A.augmix_batch(pool, recs, recipe, S, out=out)
        assert A._u8_buffers(dev, n, 3, S, False)[0] is base_c
        runs.append((out.clone(), base_c.clone(), chains_c.clone()))
    torch.cuda.synchronize()
    assert torch.isfinite(runs[0][0]).all()
    for run in runs[1:] + [A.augmix_batch(pool, recs, recipe, S, keep_u8=True)]:  # other fills; the call repeated
        for a, b in zip(run, runs[0]):
            assert torch.equal(a, b)
    for v in (0, 1, 7, 11):  # one view computed alone equals its slice of the batch
        alone = A.augmix_batch(pool, recs[v:v + 1], A.Recipe(*(t[v:v + 1] for t in recipe)), S, keep_u8=True)
        for a, b in zip(alone, runs[0]):
            assert torch.equal(a[0], b[v]), v
    side = torch.cuda.Stream(dev)
    x = torch.randn(2048, 2048, device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    for _ in range(8):  # the default stream is busy while the side stream generates
        x = x @ x * 1e-3
    with torch.cuda.stream(side):
        on_side = A.augmix_batch(pool, recs, recipe, S, keep_u8=True)
    side.synchronize()
    torch.cuda.synchronize()
    for a, b in zip(on_side, runs[0]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------- 5. public API
def test_view_groups_and_make_augmix_views(dev):
    import tta
    from PIL import Image
    from clipfs import augmix as A
    from clipfs import data
    from clipfs.views import CLIP_MEAN, CLIP_STD
    S, G, nv = 224, 2, 7
    arrays = _sources()
    pool = data.ImagePool.from_arrays(arrays, [0, 1], device=dev)
    out = A.view_groups(pool, [1, 0], n_views=nv, severity=3, seed=3, size=S)
    assert tuple(out.shape) == (G, 1 + nv, 3, S, S) and out.dtype == torch.float32
    recs, plain = A.group_records(pool, [1, 0], nv, size=S, seed=3)
    recipe = A.sample_recipes(G * (1 + nv), S, width=3, severity=3, seed=3, plain=plain)
    assert plain.reshape(G, 1 + nv)[:, 0].all() and not plain.reshape(G, 1 + nv)[:, 1:].any()
    got = out.cpu().numpy().reshape(G * (1 + nv), 3, S, S)
    for g, i in enumerate((1, 0)):
        centre = tta.make_tta_views(arrays[i], n_crops=1, size=S, device=dev)[0]
        assert torch.equal(out[g, 0], centre)
        for k in range(1, 1 + nv):
            v = g * (1 + nv) + k
            assert recs[v, 0] == i
            want = R.pil_view(arrays[i], recs[v], recipe, v, S, CLIP_MEAN, CLIP_STD)[2]
            assert np.array_equal(_bits(got[v]), _bits(want)), (g, k)
    assert not torch.equal(out[0, 1], out[0, 2])
    one = data.ImagePool.from_arrays([arrays[0]], [0], device=dev)
    want = A.view_groups(one, [0], n_views=5, severity=1, seed=9, size=S)[0]
    assert torch.equal(tta.make_augmix_views(Image.fromarray(arrays[0]), n_views=5, seed=9, size=S, device=dev), want)
    assert torch.equal(tta.make_augmix_views(arrays[0], n_views=5, seed=9, size=S, device=dev), want)


# ---------------------------------------------------------------------------------------------- 6. TDA front end
def _tda_case(dev, G=5, V=16, Cn=12, d=32, seed=3):
    import tda_ref
    T, F, _ = tda_ref.clustered(Cn, G, d, seed)
    rng = np.random.default_rng(seed + 1)
    # V views of each image: the image's feature plus noise of growing size, so the views lean towards one class with
    # entropies that differ by far more than fp32 rounding
    noise = rng.standard_normal((G, V, d)) / np.sqrt(d) * np.linspace(0.05, 0.6, V)[rng.permutation(V)][None, :, None]
    feats = tda_ref.unit(F[:, None, :] + noise).astype(np.float32)
    return torch.from_numpy(T.astype(np.float32)).to(dev), torch.from_numpy(feats).to(dev)


def _same_adapter_outcome(a, res_a, b, res_b):
    for x, y in zip(res_a, res_b):
        assert x.dtype == y.dtype and torch.equal(x, y)
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        if k != "meta":
            assert torch.equal(sa[k], sb[k]), k


def test_tda_view_front_end(dev):
    from clipfs import ops
    from tda import TestTimeDynamicAdapter
    text, feats = _tda_case(dev)
    G, V, d = feats.shape
    for rho, K in ((0.25, 4), (1.0 / V, 1), (1.0, V)):
        a, b = TestTimeDynamicAdapter(text), TestTimeDynamicAdapter(text)
        for _ in range(2):  # the second pass meets warm caches
            got = a.adapt_view_features(feats, rho=rho)
            _, sel, _, ent = ops.tpt_objective(feats, b.text, K, logit_scale=100.0, want_grad=False, want_entropy=True)
            assert tuple(sel.shape) == (G, K)
            picked = torch.gather(feats, 1, sel.long().unsqueeze(-1).expand(G, K, d))
            if K == 1:  # the single most confident view, as it stands
                assert torch.equal(sel[:, 0].long(), ent.argmin(dim=1))
                means = feats[torch.arange(G, device=dev), ent.argmin(dim=1)]
            else:
                means = picked.mean(dim=1)
            want = b.adapt_features(means)
            _same_adapter_outcome(a, got, b, want)
        assert int(a.state["counter"].item()) == 2 * G
        frozen = a.state_dict()
        a.adapt_view_features(feats, rho=rho, update=False)
        for k, t in a.state_dict().items():
            assert k == "meta" or torch.equal(t, frozen[k])
    with pytest.raises(ValueError, match="rho"):
        a.adapt_view_features(feats, rho=0.0)
    with pytest.raises(ValueError, match="expected feats"):
        a.adapt_view_features(feats[0])
    with pytest.raises(ValueError, match="without a clip_model"):
        a.adapt_views(torch.zeros(1, 2, 3, 8, 8, device=dev))


# ----------------------------------------------------------------------------- 7. the towers take view_groups' output
def test_tpt_and_tda_run_on_view_groups_through_the_small_tower(dev):
    """Shapes and finiteness only: the towers' own arithmetic is tested elsewhere."""
    import test_tpt_gpu as T
    from clipfs import augmix as A
    from clipfs import data, ops
    from tda import TestTimeDynamicAdapter
    m = T._build(dev)
    S = m.cfg.image_resolution
    arrays = _sources()
    pool = data.ImagePool.from_arrays(arrays, [0, 1], device=dev)
    views = A.view_groups(pool, [0, 1], n_views=7, severity=3, seed=1, size=S)
    assert tuple(views.shape) == (2, 8, 3, S, S) and torch.isfinite(views).all()
    res = T._tuner(m).adapt_views(views)
    Cn = m.ids.shape[0]
    assert tuple(res.logits.shape) == (2, Cn) and torch.isfinite(res.logits).all() and tuple(res.selected.shape) == (2, 2)
    text = torch.randn(Cn, m.cfg.embed_dim, generator=torch.Generator().manual_seed(0)).to(dev)
    adapter = TestTimeDynamicAdapter(text, clip_model=m.model)
    out = adapter.adapt_views(views, rho=0.25)
    assert tuple(out.logits.shape) == (2, Cn) and torch.isfinite(out.logits).all()
    f = ops.l2norm_fwd(m.model.encode_image(views.reshape(16, 3, S, S)).float().contiguous()).view(2, 8, -1)
    twin = TestTimeDynamicAdapter(text, clip_model=m.model)
    assert torch.equal(twin.adapt_view_features(f, rho=0.25).logits, out.logits)
