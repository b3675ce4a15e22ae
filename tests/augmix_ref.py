"""The oracle of the AugMix tests: a recipe applied with PIL itself (``pil_view``), and a plain numpy restatement of the five
device rules of include/clipfs.h, "AUGMIX" (``np_op``), which test_augmix_cpu.py holds against PIL bit for bit.  PIL is the
library the published AugMix / TPT / TDA pipelines call; it is not part of the oracle package."""
import numpy as np

NONE, AUTOCONTRAST, EQUALIZE, POSTERIZE, SOLARIZE, AFFINE = range(6)


def image(H, W, seed):
    """The generator of tests/test_train_crops_gpu.py::_image."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    arr = np.stack([np.sin(xx / 17.0) * 90 + 128, np.cos(yy / 23.0) * 90 + 128, (xx + yy) % 256], -1)
    return np.clip(arr + rng.randint(-30, 30, arr.shape), 0, 255).astype(np.uint8)


def pil_crop(arr, rec, size):
    """uint8 [S, S, 3] of one crop record through PIL: crop -> resize -> window -> flip (test_train_crops_gpu.py::_pil_u8,
    kept HWC)."""
    from PIL import Image
    _, top, left, h, w, flip, ow, oh, wx, wy, filt, _ = (int(v) for v in rec)
    im = Image.fromarray(arr).crop((left, top, left + w, top + h))
    im = im.resize((ow, oh), Image.BICUBIC if filt == 1 else Image.BILINEAR)
    im = im.crop((wx, wy, wx + size, wy + size))
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(im)


def pil_op(u8, code, param, coef):
    """One operation on a uint8 [S, S, 3] image through PIL."""
    from PIL import Image, ImageOps
    im = Image.fromarray(u8)
    S = u8.shape[0]
    if code == NONE:
        out = im
    elif code == AUTOCONTRAST:
        out = ImageOps.autocontrast(im)
    elif code == EQUALIZE:
        out = ImageOps.equalize(im)
    elif code == POSTERIZE:
        out = ImageOps.posterize(im, int(param))
    elif code == SOLARIZE:
        out = ImageOps.solarize(im, int(param))
    elif code == AFFINE:
        out = im.transform((S, S), Image.AFFINE, tuple(float(c) for c in coef), resample=Image.BILINEAR)
    else:
        raise ValueError(code)
    return np.asarray(out)


def chain(u8, ops, coef, depth, op=pil_op):
    for s in range(int(depth)):
        u8 = op(u8, int(ops[s, 0]), int(ops[s, 1]), coef[s])
    return u8


def normalise(u8_hwc, mean, std):
    """t(u) of the rule in float32, operation for operation, as [3, S, S]."""
    f32 = np.float32
    mean = np.asarray(mean, f32).reshape(-1, 1, 1)
    std = np.asarray(std, f32).reshape(-1, 1, 1)
    return (u8_hwc.transpose(2, 0, 1).astype(f32) - mean * f32(255)) * ((f32(1) / f32(255)) / std)


def mix(base, chains, w, m, mean, std):
    """out = m t(base) + (1 - m) sum_i w_i t(chain_i) in float32, every operation rounded on its own, chains ascending."""
    f32 = np.float32
    acc = np.zeros((3,) + base.shape[:2], f32)
    for i, c in enumerate(chains):
        acc = acc + f32(w[i]) * normalise(c, mean, std)
    return f32(m) * normalise(base, mean, std) + (f32(1) - f32(m)) * acc


def pil_view(arr, rec, recipe, v, size, mean, std, op=pil_op):
    """(base_u8 [S, S, 3], chains_u8 [width, S, S, 3], out fp32 [3, S, S]) of view ``v`` of a recipe on source ``arr``."""
    base = pil_crop(arr, rec, size)
    width = recipe.depth.shape[1]
    chains = [chain(base, recipe.ops[v, i], recipe.coef[v, i], recipe.depth[v, i], op) for i in range(width)]
    return base, np.stack(chains), mix(base, chains, recipe.w[v], recipe.m[v], mean, std)


# ------------------------------------------------------------------------------------- the device rules, in plain numpy
def _lut_autocontrast(h):
    nz = np.nonzero(h)[0]
    lo, hi = int(nz[0]), int(nz[-1])
    if hi <= lo:
        return np.arange(256)
    scale = np.float64(255.0) / np.float64(hi - lo)
    offset = np.float64(-lo) * scale
    return np.clip((np.arange(256, dtype=np.float64) * scale + offset).astype(np.int64), 0, 255)  # astype: towards zero


def _lut_equalize(h):
    nz = h[h != 0]
    step = (int(h.sum()) - int(nz[-1])) // 255
    if len(nz) <= 1 or step == 0:
        return np.arange(256)
    n = step // 2 + np.concatenate([[0], np.cumsum(h[:-1])])
    return np.minimum(n // step, 255)


def np_affine(u8, a):
    S = u8.shape[0]
    a = [np.float64(c) for c in a]
    yy, xx = np.mgrid[0:S, 0:S]
    xc, yc = xx + np.float64(0.5), yy + np.float64(0.5)
    xin = a[0] * xc + a[1] * yc + a[2]
    yin = a[3] * xc + a[4] * yc + a[5]
    inside = ~((xin < 0) | (xin >= S) | (yin < 0) | (yin >= S))
    xin, yin = np.where(inside, xin, 0.5) - 0.5, np.where(inside, yin, 0.5) - 0.5
    X, Y = np.floor(xin), np.floor(yin)
    dx, dy = (xin - X)[..., None], (yin - Y)[..., None]
    X, Y = X.astype(np.int64), Y.astype(np.int64)
    x0, x1, y0 = np.clip(X, 0, S - 1), np.clip(X + 1, 0, S - 1), np.clip(Y, 0, S - 1)
    img = u8.astype(np.float64)
    v1 = img[y0, x0] + (img[y0, x1] - img[y0, x0]) * dx
    two = (Y + 1 >= 0) & (Y + 1 < S)
    y1 = np.where(two, Y + 1, 0)
    v2 = np.where(two[..., None], img[y1, x0] + (img[y1, x1] - img[y1, x0]) * dx, v1)
    out = (v1 + (v2 - v1) * dy).astype(np.int64)
    return np.where(inside[..., None], out, 0).astype(np.uint8)


def np_op(u8, code, param, coef):
    """One operation by the written rule (what csrc/augmix.hip restates on the device)."""
    if code == NONE:
        return u8.copy()
    if code in (AUTOCONTRAST, EQUALIZE):
        out = np.empty_like(u8)
        for c in range(3):
            h = np.bincount(u8[..., c].reshape(-1), minlength=256)
            lut = _lut_autocontrast(h) if code == AUTOCONTRAST else _lut_equalize(h)
            out[..., c] = lut[u8[..., c]]
        return out
    if code == POSTERIZE:
        return u8 & np.uint8(~((1 << (8 - int(param))) - 1) & 255)
    if code == SOLARIZE:
        return np.where(u8.astype(np.int64) < int(param), u8, 255 - u8).astype(np.uint8)
    if code == AFFINE:
        return np_affine(u8, coef)
    raise ValueError(code)


# ------------------------------------------------------------------------------------------------ the edge-case images
def edge_cases(S):
    """[(name, uint8 [S, S, 3] image, code, param, coef)]: every case of the GPU test's "each operation alone" list that
    makes sense at side S."""
    from clipfs import augmix as A
    rng = np.random.RandomState(S)
    noisy = rng.randint(0, 256, (S, S, 3)).astype(np.uint8)
    full = image(S, S, 40 + S)
    full[0, 0], full[0, 1] = 0, 255
    narrow = (40 + rng.randint(0, 51, (S, S, 3))).astype(np.uint8)
    const = noisy.copy()
    const[..., 1] = 77  # a constant channel
    few = np.full((S, S, 3), 200, np.uint8)  # so few pixels below the top bin that step == 0 at every S
    few[0, :3] = (3, 150, 17)
    ident = A.IDENTITY
    cases = [("autocontrast-full", full, AUTOCONTRAST, 0, ident), ("autocontrast-narrow", narrow, AUTOCONTRAST, 0, ident),
             ("autocontrast-const", const, AUTOCONTRAST, 0, ident), ("equalize-noisy", noisy, EQUALIZE, 0, ident),
             ("equalize-const", const, EQUALIZE, 0, ident), ("equalize-few", few, EQUALIZE, 0, ident),
             ("equalize-smooth", full, EQUALIZE, 0, ident)]
    cases += [(f"posterize-{b}", noisy, POSTERIZE, b, ident) for b in (1, 4, 8)]
    cases += [(f"solarize-{t}", noisy, SOLARIZE, t, ident) for t in (0, 128, 256)]
    cases += [(f"rotate{d:+d}", full, AFFINE, 0, A.rotate_coefficients(d, S)) for d in (0, 7, -30)]
    for sgn in (0.3, -0.3):
        cases.append((f"shear_x{sgn:+}", full, AFFINE, 0, (1.0, sgn, 0.0, 0.0, 1.0, 0.0)))
        cases.append((f"shear_y{sgn:+}", noisy, AFFINE, 0, (1.0, 0.0, 0.0, sgn, 1.0, 0.0)))
    t = float(int(S / 3))
    for d in (0.0, t, -t, 2.25):
        cases.append((f"translate_x{d:+}", noisy, AFFINE, 0, (1.0, 0.0, d, 0.0, 1.0, 0.0)))
        cases.append((f"translate_y{d:+}", full, AFFINE, 0, (1.0, 0.0, 0.0, 0.0, 1.0, d)))
    cases.append(("affine-all-outside", noisy, AFFINE, 0, (1.0, 0.0, 10.0 * S, 0.0, 1.0, -10.0 * S)))
    return cases
