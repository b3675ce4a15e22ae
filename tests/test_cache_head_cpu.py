"""Host-only checks of the Tip-Adapter cache head: clipfs_cache_plan (the function clipfs_cache_logits, _bwd and _search
execute) for the bench geometries and the edge shapes of the GPU suite, every refusal from the plan and from the entry
points (NULL stream, nothing launched), and TipAdapter.from_features on CPU tensors."""
import ctypes

import pytest
import torch

LDS_LIMIT = 160 * 1024
SHOTS = [0, 1, 3, 16, 40, 2, 5, 7, 33, 4, 1, 9]
# (B, NK, C, d, nA, nB): the two bench geometries, then the edge shapes of tests/test_cache_head_gpu.py
SHAPES = [(256, 1612, 403, 512, 20, 200), (8192, 16000, 1000, 1024, 20, 200),
          (1, 121, 12, 20, 1, 1), (37, 121, 12, 64, 5, 6), (96, 121, 12, 100, 1, 6), (300, 1612, 403, 512, 5, 1),
          (150, 121, 12, 64, 5, 25), (5, 1, 1, 4, 1024, 1024), (2048, 4096, 64, 64, 300, 7), (3, 7, 9, 4096, 257, 3)]
OPS = ("logits", "bwd_dk", "bwd_df", "search")


@pytest.fixture(scope="module")
def lib():
    from clipfs import _lib
    return _lib.load()


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_plan_covers_the_problem(shape):
    from clipfs import ops
    B, NK, C, d, nA, nB = shape
    for op in OPS:
        p = ops.cache_plan(op, B, NK, C, d, nA, nB)
        gx, gy, gz = p["grid"]
        assert p["block"] == 256 and 0 < p["lds_bytes"] <= LDS_LIMIT, (op, p)
        assert p["work_floats"] == 0
        assert min(gx, gy, gz) >= 1 and gy <= 65535 and gz <= 65535
        if op == "logits":
            assert gx * 32 >= B > (gx - 1) * 32
            cc = p["class_chunk"]
            assert cc >= 1 and gy * cc >= C > (gy - 1) * cc  # the class chunks cover C exactly once
        elif op in ("bwd_dk", "bwd_df"):
            own = NK if op == "bwd_dk" else B
            fc = p["feat_chunk"]
            assert fc in (128, 512) and gx * 32 >= own > (gx - 1) * 32 and gy * fc >= d > (gy - 1) * fc
        else:
            jb, ac = p["beta_chunk"], p["alpha_chunk"]
            assert gx * 32 >= B > (gx - 1) * 32
            assert 1 <= jb <= nB and gy * jb >= nB > (gy - 1) * jb  # the beta chunks cover nB exactly
            assert 1 <= ac <= nA and gz * ac >= nA > (gz - 1) * ac
            # the records, carries and the two key tiles the kernel lays out must fit what the plan asks for
            need = 4 * (2 * 128 * 32 + 2 * jb * ac * 32 + jb * 32 + ac + jb + 3 * 128 + 1)
            assert need <= p["lds_bytes"]


def test_plan_is_a_pure_function():
    from clipfs import ops
    a = ops.cache_plan("search", 8192, 16000, 1000, 1024, 20, 200)
    assert a == ops.cache_plan("search", 8192, 16000, 1000, 1024, 20, 200)
    assert a["beta_chunk"] * a["grid"][1] >= 200 and a["alpha_chunk"] == 20


BAD_SHAPES = [  # (B, NK, C, d, nA, nB), the word the message must carry
    ((0, 8, 2, 64, 1, 1), b"B"), ((4, 0, 2, 64, 1, 1), b"NK"), ((4, 8, 0, 64, 1, 1), b"C ="),
    ((4, 8, 2, 66, 1, 1), b"d ="), ((4, 8, 2, 0, 1, 1), b"d ="), ((4, 8, 2, 4100, 1, 1), b"d ="),
    ((4, 8, 2, 64, 0, 1), b"nA"), ((4, 8, 2, 64, 1025, 1), b"nA"), ((4, 8, 2, 64, 1, 0), b"nB"),
    ((4, 8, 2, 64, 1, 1025), b"nB"),
]


@pytest.mark.parametrize("shape,word", BAD_SHAPES, ids=[w.decode().strip(" =") + str(i) for i, (_, w) in enumerate(BAD_SHAPES)])
def test_plan_refusals_name_the_argument(lib, shape, word):
    from clipfs import _lib
    for op in range(4):
        plan = _lib.CachePlan()
        plan.block = 77
        assert lib.clipfs_cache_plan(op, *shape, ctypes.byref(plan)) == 1
        assert word in lib.clipfs_last_error(), lib.clipfs_last_error()
        assert plan.block == 77  # nothing written on refusal
    with pytest.raises(_lib.ClipfsError):
        _lib.cache_plan("logits", *shape)


def test_plan_refuses_unknown_op_and_null_plan(lib):
    from clipfs import _lib
    assert lib.clipfs_cache_plan(0, 4, 8, 2, 64, 1, 1, None) == 1 and b"plan" in lib.clipfs_last_error()
    assert lib.clipfs_cache_plan(9, 4, 8, 2, 64, 1, 1, ctypes.byref(_lib.CachePlan())) == 1
    assert b"op" in lib.clipfs_last_error()


def test_entry_points_refuse_before_launching(lib):
    """Fake (never dereferenced) device addresses, a NULL stream: every refusal returns CLIPFS_EINVAL with its cause."""
    f, K, off, base, out, dl, dK, df, y, al, be, hits = (0x10000 * (i + 1) for i in range(12))
    B, NK, C, d = 4, 8, 2, 64

    def logits(f=f, K=K, base=base, out=out, B=B, NK=NK, C=C, d=d, ldb=C, ldo=C, alpha=1.0, beta=5.5):
        return lib.clipfs_cache_logits(f, K, off, base, out, B, NK, C, d, ldb, ldo, alpha, beta, None)

    def bwd(f=f, K=K, dK=dK, df=df, B=B, d=d, ldd=C, alpha=1.0, beta=5.5):
        return lib.clipfs_cache_bwd(f, K, off, dl, dK, df, B, NK, C, d, ldd, alpha, beta, None)

    def search(f=f, K=K, B=B, d=d, ldb=C, nA=3, nB=2):
        return lib.clipfs_cache_search(f, K, off, base, y, al, be, hits, B, NK, C, d, ldb, nA, nB, None)

    def refused(rc, word):
        assert rc == 1 and word in lib.clipfs_last_error(), (rc, lib.clipfs_last_error())

    for call in (logits, bwd, search):
        refused(call(f=None), b"f is")
        refused(call(f=f + 4), b"f is")
        refused(call(K=None), b"K is")
        refused(call(K=K + 8), b"K is")
        refused(call(d=6), b"d =")
        refused(call(d=8192), b"d =")
        refused(call(B=0), b"B =")
    refused(logits(out=None), b"out")
    refused(logits(out=out + 4), b"out")
    refused(logits(NK=0), b"NK")
    refused(logits(C=0), b"C =")
    refused(logits(ldo=C - 1), b"ldout")
    refused(logits(ldb=C - 1), b"ldbase")
    refused(logits(out=base), b"alias")
    refused(bwd(dK=None), b"dK")
    refused(bwd(dK=dK + 12), b"dK")
    refused(bwd(df=df + 4), b"df")
    refused(bwd(ldd=1), b"lddl")
    refused(search(ldb=1), b"ldbase")
    refused(search(nA=0), b"nA")
    refused(search(nA=1025), b"nA")
    refused(search(nB=0), b"nB")
    refused(search(nB=2000), b"nB")
    for call in (logits, bwd):
        for bad in (-1.0, float("nan"), float("inf")):
            refused(call(alpha=bad), b"alpha")
            refused(call(beta=bad), b"beta")


def test_from_features_sorts_stably_by_class():
    from tip_adapter import TipAdapter
    g = torch.Generator().manual_seed(3)
    labels = torch.tensor([4, 1, 4, 0, 6, 1, 4, 0, 1, 6, 4])  # classes 2, 3, 5 (middle) and 7 (last) own no key
    feats = torch.nn.functional.normalize(torch.randn(labels.numel(), 8, generator=g), dim=1)
    ad = TipAdapter.from_features(feats, labels, n_classes=8, alpha=2.0, beta=3.0)
    assert ad.order.tolist() == [3, 7, 1, 5, 8, 0, 2, 6, 10, 4, 9]  # equal labels keep the caller's order
    assert ad.labels.tolist() == [0, 0, 1, 1, 1, 4, 4, 4, 4, 6, 6]
    assert ad.offsets.dtype == torch.int32 and ad.offsets.tolist() == [0, 2, 5, 5, 5, 9, 9, 11, 11]
    assert torch.equal(ad.keys.detach(), feats[ad.order]) and ad.keys.requires_grad
    back = torch.empty_like(feats)
    back[ad.order] = ad.keys.detach()  # order inverts the sort
    assert torch.equal(back, feats)
    assert ad.n_classes == 8 and (ad.alpha, ad.beta) == (2.0, 3.0)
    # an empty FIRST class
    ad = TipAdapter.from_features(feats, labels + 1, n_classes=9)
    assert ad.offsets.tolist() == [0, 0, 2, 5, 5, 5, 9, 9, 11, 11]


def test_state_dict_round_trip_and_refusals():
    from tip_adapter import TipAdapter
    feats = torch.nn.functional.normalize(torch.randn(6, 8, generator=torch.Generator().manual_seed(1)), dim=1)
    labels = torch.tensor([2, 0, 1, 2, 0, 2])
    a = TipAdapter.from_features(feats, labels, 3, alpha=0.75, beta=6.5)
    b = TipAdapter.from_features(torch.roll(feats, 1, 0), torch.tensor([0, 0, 0, 1, 1, 2]), 3)
    b.load_state_dict(a.state_dict())
    assert torch.equal(b.keys, a.keys) and torch.equal(b.offsets, a.offsets) and torch.equal(b.order, a.order)
    assert torch.equal(b.labels, a.labels) and (b.alpha, b.beta) == (0.75, 6.5)
    with pytest.raises(ValueError):
        TipAdapter.from_features(feats, labels, 2)  # label 2 outside [0, 2)
    with pytest.raises(ValueError):
        TipAdapter.from_features(feats[:, :6], labels, 3)  # width not a multiple of 4
