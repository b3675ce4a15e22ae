"""AugMix without a GPU: the recipe sampler (clipfs/augmix.py), the rotate coefficients against Image.rotate, and the numpy
restatement of the five device rules (tests/augmix_ref.py) against PIL, bit for bit, on the edge cases the GPU tests run."""
import numpy as np
import pytest

import augmix_ref as R
from clipfs import augmix as A


def test_sampler_is_deterministic_and_shaped():
    a = A.sample_recipes(20, 224, width=3, severity=3, seed=5)
    b = A.sample_recipes(20, 224, width=3, severity=3, seed=5)
    c = A.sample_recipes(20, 224, width=3, severity=3, seed=6)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert not np.array_equal(a.coef, c.coef) and not np.array_equal(a.w, c.w)
    assert a.ops.shape == (20, 3, 3, 2) and a.ops.dtype == np.int32
    assert a.coef.shape == (20, 3, 3, 6) and a.coef.dtype == np.float64
    assert a.depth.shape == (20, 3) and a.depth.dtype == np.int32
    assert a.w.shape == (20, 3) and a.w.dtype == np.float32 and a.m.shape == (20,) and a.m.dtype == np.float32
    assert a.depth.min() >= 1 and a.depth.max() <= 3
    assert np.all((a.m >= 0) & (a.m <= 1)) and np.all(a.w >= 0)
    assert np.abs(a.w.astype(np.float64).sum(1) - 1).max() <= 3 * 2.0 ** -24  # three fp32 roundings of numbers below 1
    one = A.sample_recipes(4, 37, width=1, max_depth=1, seed=1)
    assert one.depth.tolist() == [[1]] * 4 and np.all(one.w == 1)


@pytest.mark.parametrize("severity", [1, 3, 10])
def test_levels_stay_inside_the_published_ranges(severity):
    S = 224
    r = A.sample_recipes(300, S, width=3, severity=severity, seed=severity)
    seen = set()
    for v in range(300):
        for i in range(3):
            for s in range(r.depth[v, i]):
                code, param = r.ops[v, i, s]
                co = r.coef[v, i, s]
                seen.add(int(code))
                assert 1 <= code <= 5
                if code == A.POSTERIZE:
                    assert max(1, 4 - int(severity * 4 / 10)) <= param <= 4
                elif code == A.SOLARIZE:
                    assert 256 - int(severity * 256 / 10) <= param <= 256
                elif code == A.AFFINE:
                    assert np.all(np.isfinite(co))
                    if co[0] != 1.0 or co[4] != 1.0:  # a rotation by at most int(severity * 3) degrees
                        assert co[0] == co[4] and co[1] == -co[3] and co[0] >= round(np.cos(np.radians(int(severity * 3))), 15)
                    else:
                        assert abs(co[1]) <= severity * 0.03 and abs(co[3]) <= severity * 0.03  # shear
                        assert abs(co[2]) <= int(severity * (S / 3) / 10) and abs(co[5]) <= int(severity * (S / 3) / 10)
                        assert co[2] == int(co[2]) and co[5] == int(co[5])  # whole pixels
                else:
                    assert param == 0 and tuple(co) == A.IDENTITY
    assert seen == {1, 2, 3, 4, 5}


def test_plain_views_and_refusals():
    plain = np.array([True, False, False, True])
    r = A.sample_recipes(4, 224, seed=2, plain=plain)
    free = A.sample_recipes(4, 224, seed=2)
    assert np.all(r.m[plain] == 1) and np.all(r.depth[plain] == 0) and np.all(r.ops[plain] == 0)
    for x, y in zip(r, free):  # a plain view consumes the same random numbers: the others do not move
        assert np.array_equal(x[~plain], y[~plain])
    assert np.array_equal(r.w, free.w)
    for kw in (dict(n=0), dict(S=225), dict(S=7), dict(width=5), dict(max_depth=4), dict(severity=11), dict(op_names=("blur",)),
               dict(plain=[True])):
        with pytest.raises(ValueError):
            A.sample_recipes(**{**dict(n=4, S=224), **kw})


@pytest.mark.parametrize("angle", [0, 7, -7, -30, 30, 1, 90, 123.5])
def test_rotate_coefficients_reproduce_image_rotate(angle):
    from PIL import Image
    im = Image.fromarray(R.image(37, 37, 3))
    want = np.asarray(im.rotate(angle, Image.BILINEAR))
    got = np.asarray(im.transform((37, 37), Image.AFFINE, A.rotate_coefficients(angle, 37), resample=Image.BILINEAR))
    assert np.array_equal(got, want)


@pytest.mark.parametrize("S", [224, 37, 8])
def test_written_rule_equals_pil_on_the_edge_cases(S):
    cases = R.edge_cases(S)
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names) and len(cases) == 29
    for name, u8, code, param, coef in cases:
        want = R.pil_op(u8, code, param, coef)
        got = R.np_op(u8, code, param, coef)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (S, name, int(np.abs(got.astype(int) - want).max()))
    by = {c[0]: c for c in cases}
    # the cases are what they claim to be
    h = np.bincount(by["equalize-noisy"][1][..., 0].reshape(-1), minlength=256)
    step = (int(h.sum()) - int(h[h != 0][-1])) // 255
    if S >= 37:
        assert step > 0 and R.np_op(by["equalize-noisy"][1], R.EQUALIZE, 0, None).max() == 255
    else:
        assert step == 0  # 64 pixels per channel
    h = np.bincount(by["equalize-few"][1][..., 0].reshape(-1), minlength=256)
    assert (h != 0).sum() > 1 and (int(h.sum()) - int(h[h != 0][-1])) // 255 == 0  # several bins, step == 0
    assert np.array_equal(R.np_op(by["equalize-few"][1], R.EQUALIZE, 0, None), by["equalize-few"][1])
    assert np.array_equal(R.np_op(by["autocontrast-const"][1], R.AUTOCONTRAST, 0, None)[..., 1], by["autocontrast-const"][1][..., 1])
    assert not R.np_op(by["affine-all-outside"][1], R.AFFINE, 0, by["affine-all-outside"][4]).any()
    t = int(S / 3)
    moved = R.np_op(by[f"translate_x{float(t):+}"][1], R.AFFINE, 0, by[f"translate_x{float(t):+}"][4])
    assert not moved[:, S - t:].any() and np.array_equal(moved[:, :S - t], by[f"translate_x{float(t):+}"][1][:, t:])


def test_written_rule_equals_pil_on_random_chains():
    """Whole sampled recipes, operation after operation (EQUALIZE after AFFINE sees the fill)."""
    S = 37
    r = A.sample_recipes(24, S, width=3, severity=10, seed=9)
    base = R.image(S, S, 12)
    for v in range(24):
        for i in range(3):
            want = R.chain(base, r.ops[v, i], r.coef[v, i], r.depth[v, i], R.pil_op)
            got = R.chain(base, r.ops[v, i], r.coef[v, i], r.depth[v, i], R.np_op)
            assert np.array_equal(got, want), (v, i, r.ops[v, i].tolist())


def test_module_states_what_is_not_offered():
    for phrase in ("ImageEnhance", "S above 224", "Jensen-Shannon", "sampled on the device"):
        assert phrase in A.__doc__, phrase
