"""AugMix test-time views made on the GPU from a device-resident image pool (csrc/augmix.hip; the rule: include/clipfs.h,
"AUGMIX").

AugMix (Hendrycks et al., ICLR 2020) is what test-time prompt tuning and TDA are published with: a view is a random resized
crop, ``width`` chains of one to three PIL operations on it, and a convex mix of the normalised chains with the normalised
crop.  The published pipelines run it with PIL on the host, about six PIL calls per view.  Here the host only samples the
recipe (``sample_recipes``: integers and a few doubles per view) and one call of ``augmix_batch`` writes the views; every
uint8 image on the way equals PIL's bit for bit.

    sample_recipes   the five recipe tables of a batch of views, from np.random.RandomState(seed)
    augmix_batch     one call of clipfs_augmix_batch on the current stream
    view_groups      [G, 1 + n_views, 3, S, S]: a plain centre view and n_views AugMix views per pool image, the tensor
                     ``TestTimePromptTuner.adapt_views`` and ``TestTimeDynamicAdapter.adapt_views`` take

Not offered: the four ImageEnhance operations of AugMix's full list (color, contrast, brightness, sharpness; TPT leaves them
out too), S above 224, a Jensen-Shannon training loss, recipes sampled on the device.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import check
from .data import REC_COLS, ImagePool
from .views import BILINEAR, CLIP_MEAN, CLIP_STD, centre_view_record, sample_crop

NONE, AUTOCONTRAST, EQUALIZE, POSTERIZE, SOLARIZE, AFFINE = range(6)  # CLIPFS_AUGMIX_* of include/clipfs.h
AUGMIX_OPS = ("autocontrast", "equalize", "posterize", "rotate", "solarize", "shear_x", "shear_y", "translate_x",
              "translate_y")
MAX_SIZE, MIN_SIZE, MAX_WIDTH, MAX_DEPTH, MAX_VIEWS = 224, 8, 4, 3, 65536  # the limits of clipfs_augmix_batch
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


class Recipe(NamedTuple):
    ops: np.ndarray    # int32 [n, width, 3, 2] = {code, param}
    coef: np.ndarray   # float64 [n, width, 3, 6], the affine coefficients of AFFINE steps (identity elsewhere)
    depth: np.ndarray  # int32 [n, width], operations per chain
    w: np.ndarray      # fp32 [n, width], the chain weights
    m: np.ndarray      # fp32 [n], the weight of the unaugmented crop


def rotate_coefficients(angle: float, size: int):
    """The six coefficients ``Image.rotate(angle, BILINEAR)`` hands to ``Image.transform`` for a size x size image."""
    a = -math.radians(angle % 360.0)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    cx = cy = size / 2
    x, y = -cx, -cy
    m[2], m[5] = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2] += cx
    m[5] += cy
    return tuple(m)


def op_step(name: str, level: float, negate: bool, size: int):
    """One published AugMix operation at ``level`` (in [0, 10]) -> (code, param, six coefficients).  ``negate`` is the coin
    of the signed operations."""
    int_parameter = lambda maxval: int(level * maxval / 10)
    float_parameter = lambda maxval: float(level) * maxval / 10.0
    sign = -1.0 if negate else 1.0
    if name == "autocontrast":
        return AUTOCONTRAST, 0, IDENTITY
    if name == "equalize":
        return EQUALIZE, 0, IDENTITY
    if name == "posterize":
        return POSTERIZE, max(4 - int_parameter(4), 1), IDENTITY  # bits 0 (level exactly 10) is not an image operation
    if name == "solarize":
        return SOLARIZE, 256 - int_parameter(256), IDENTITY
    if name == "rotate":
        return AFFINE, 0, rotate_coefficients(sign * int_parameter(30), size)
    if name == "shear_x":
        return AFFINE, 0, (1.0, sign * float_parameter(0.3), 0.0, 0.0, 1.0, 0.0)
    if name == "shear_y":
        return AFFINE, 0, (1.0, 0.0, 0.0, sign * float_parameter(0.3), 1.0, 0.0)
    if name == "translate_x":
        return AFFINE, 0, (1.0, 0.0, sign * int_parameter(size / 3), 0.0, 1.0, 0.0)
    if name == "translate_y":
        return AFFINE, 0, (1.0, 0.0, 0.0, 0.0, 1.0, sign * int_parameter(size / 3))
    raise ValueError(f"unknown AugMix operation {name!r}; known: {', '.join(AUGMIX_OPS)}")


_SIGNED = ("rotate", "shear_x", "shear_y", "translate_x", "translate_y")


def sample_recipes(n: int, S: int, width: int = 3, max_depth: int = 3, severity: float = 1, seed: int = 0,
                   op_names: Sequence[str] = AUGMIX_OPS, plain=None) -> Recipe:
    """The recipe tables of ``n`` views of side ``S``, a function of the arguments alone.  Per view w ~ Dirichlet(1, .., 1)
    and m ~ Beta(1, 1); per chain depth ~ randint(1, max_depth + 1); per step a uniformly chosen name of ``op_names`` at
    level ~ U(0.1, severity) with the published parameter maps (rotate int(level 30 / 10) degrees, posterize
    4 - int(level 4 / 10) bits, solarize 256 - int(level 256 / 10), shear level 0.3 / 10, translate int(level (S / 3) / 10)
    pixels; the sign of the five geometric operations flips with probability 1/2).  ``plain``: a boolean mask [n]; a plain
    view has m = 1 and all depths 0 (it is the crop), and consumes the same random numbers as any other view."""
    if not (1 <= n <= MAX_VIEWS and MIN_SIZE <= S <= MAX_SIZE and 1 <= width <= MAX_WIDTH and 1 <= max_depth <= MAX_DEPTH):
        raise ValueError(f"sample_recipes: n {n} in [1, {MAX_VIEWS}], S {S} in [{MIN_SIZE}, {MAX_SIZE}], width {width} in "
                         f"[1, {MAX_WIDTH}], max_depth {max_depth} in [1, {MAX_DEPTH}]")
    if not 0.1 <= severity <= 10:
        raise ValueError(f"sample_recipes: severity {severity} must be in [0.1, 10]")
    op_names = tuple(op_names)
    for name in op_names:
        op_step(name, 1.0, False, S)  # ValueError for an unknown name
    plain = np.zeros(n, dtype=bool) if plain is None else np.asarray(plain, dtype=bool).reshape(-1)
    if plain.shape[0] != n:
        raise ValueError(f"sample_recipes: plain has {plain.shape[0]} entries for {n} views")
    rng = np.random.RandomState(seed)
    ops = np.zeros((n, width, 3, 2), dtype=np.int32)
    coef = np.tile(np.asarray(IDENTITY, dtype=np.float64), (n, width, 3, 1))
    depth = np.zeros((n, width), dtype=np.int32)
    w = np.zeros((n, width), dtype=np.float32)
    m = np.zeros(n, dtype=np.float32)
    for v in range(n):
        w[v] = rng.dirichlet([1.0] * width).astype(np.float32)
        m[v] = np.float32(rng.beta(1.0, 1.0))
        for i in range(width):
            depth[v, i] = rng.randint(1, max_depth + 1)
            for s in range(depth[v, i]):
                name = op_names[rng.randint(len(op_names))]
                level = rng.uniform(0.1, severity)
                negate = bool(rng.random_sample() > 0.5) if name in _SIGNED else False
                code, param, co = op_step(name, level, negate, S)
                ops[v, i, s] = (code, param)
                coef[v, i, s] = co
        if plain[v]:
            m[v], depth[v], ops[v], coef[v] = 1.0, 0, 0, IDENTITY
    return Recipe(ops, coef, depth, w, m)


_U8_CACHE = {}


def _u8_buffers(dev, n, width, S, keep):
    plan = _lib.augmix_plan(n, S, width)
    key = (str(dev), n, width, S)
    hit = None if keep else _U8_CACHE.get(key)
    if hit is None:
        hit = (torch.empty(plan["base_bytes"], dtype=torch.uint8, device=dev).view(n, S, S, 3),
               torch.empty(plan["chains_bytes"], dtype=torch.uint8, device=dev).view(n, width, S, S, 3))
        if not keep:
            _U8_CACHE.clear()  # one shape at a time: the buffers of a 512-view call are 0.3 GB
            _U8_CACHE[key] = hit
    return hit


def augmix_batch(pool: ImagePool, recs: np.ndarray, recipe: Recipe, size: int = 224, out: Optional[torch.Tensor] = None,
                 keep_u8: bool = False, mean: Sequence[float] = CLIP_MEAN, std: Sequence[float] = CLIP_STD):
    """One call of clipfs_augmix_batch on the current stream: int32 [n, 12] crop records (those of ``data.crop_batch``) and
    a ``Recipe`` -> fp32 [n, 3, size, size] views on the pool's device (``out`` when given).  The tables are uploaded pinned
    and non-blocking, in one copy.  ``keep_u8``: returns (out, base_u8 [n, S, S, 3], chains_u8 [n, width, S, S, 3]) with
    buffers of the call's own; otherwise the two uint8 buffers are cached per (n, width, size) and reused by the next call
    of that shape on the same stream order."""
    from .views import _norm_constants
    recs = np.ascontiguousarray(recs, dtype=np.int32)
    if recs.ndim != 2 or recs.shape[1] != REC_COLS:
        raise ValueError(f"augmix_batch: records must be int32 [n, {REC_COLS}], got {recs.shape}")
    n, S = recs.shape[0], int(size)
    if recipe.depth.ndim != 2 or recipe.depth.shape[0] != n:
        raise ValueError(f"augmix_batch: the recipe is for {recipe.depth.shape[0] if recipe.depth.ndim else 0} views, the records for {n}")
    width = recipe.depth.shape[1]
    want = dict(ops=((n, width, 3, 2), np.int32), coef=((n, width, 3, 6), np.float64), depth=((n, width), np.int32),
                w=((n, width), np.float32), m=((n,), np.float32))
    for name, (shape, dtype) in want.items():
        t = getattr(recipe, name)
        if tuple(t.shape) != shape or t.dtype != dtype:
            raise ValueError(f"augmix_batch: recipe.{name} must be {np.dtype(dtype).name} {list(shape)}, got {t.dtype} {list(t.shape)}")
    dev = pool.device
    if out is None:
        out = torch.empty(n, 3, S, S, device=dev, dtype=torch.float32)
    elif tuple(out.shape) != (n, 3, S, S) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"augmix_batch: out must be a contiguous fp32 [{n}, 3, {S}, {S}] tensor on {dev}")
    base_u8, chains_u8 = _u8_buffers(dev, n, width, S, keep_u8)
    # one pinned blob (coef first: 8-byte alignment), one non-blocking upload; the library validates the host pointers
    parts = [np.ascontiguousarray(getattr(recipe, k)).view(np.uint8).reshape(-1) for k in ("coef", "ops", "depth", "w", "m")]
    parts.append(recs.view(np.uint8).reshape(-1))
    offs = np.cumsum([0] + [p.size for p in parts])
    host = torch.from_numpy(np.concatenate(parts)).pin_memory()
    blob = host.to(dev, non_blocking=True)
    rc = _lib.AugmixRecipe()
    rc.struct_size = C.sizeof(_lib.AugmixRecipe)
    for k, name in enumerate(("coef", "ops", "depth", "w", "m")):
        setattr(rc, name, host.data_ptr() + int(offs[k]))
        setattr(rc, name + "_dev", blob.data_ptr() + int(offs[k]))
    mu, sd = _norm_constants(dev, tuple(float(v) for v in mean), tuple(float(v) for v in std))
    check(_lib.load().clipfs_augmix_batch(pool.data.data_ptr(), pool.data.numel(), pool.table.ctypes.data,
                                          pool.table_dev.data_ptr(), len(pool), host.data_ptr() + int(offs[5]),
                                          blob.data_ptr() + int(offs[5]), n, S, width, C.byref(rc), mu.data_ptr(),
                                          sd.data_ptr(), base_u8.data_ptr(), chains_u8.data_ptr(), out.data_ptr(),
                                          torch.cuda.current_stream(dev).cuda_stream), "augmix_batch")
    return (out, base_u8, chains_u8) if keep_u8 else out


def group_records(pool: ImagePool, indices: Sequence[int], n_views: int, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0),
                  size: int = 224, seed: int = 0, flip_p: float = 0.5):
    """int32 [G (1 + n_views), 12] crop records and the boolean ``plain`` mask of ``view_groups``: per image the bicubic
    centre view (``views.centre_view_record``), then ``n_views`` RandomResizedCrop(scale) + flip boxes."""
    rng = np.random.RandomState([int(seed) & 0xFFFFFFFF, 0x41554758])
    recs, plain = [], []
    for i in indices:
        h, w = pool.size(int(i))
        recs.append((int(i),) + centre_view_record(w, h, 256, size) + (0,))
        plain.append(True)
        for _ in range(n_views):
            top, left, bh, bw = sample_crop(w, h, scale, ratio, rng)
            flip = int(rng.random_sample() < flip_p)
            recs.append((int(i), top, left, bh, bw, flip, size, size, 0, 0, BILINEAR, 0))
            plain.append(False)
    return np.asarray(recs, dtype=np.int32).reshape(-1, REC_COLS), np.asarray(plain, dtype=bool)


def view_groups(pool: ImagePool, indices: Sequence[int], n_views: int = 63, scale=(0.08, 1.0), severity: float = 1,
                width: int = 3, seed: int = 0, size: int = 224, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 [G, 1 + n_views, 3, size, size] for the pool images ``indices``: view 0 of an image is its plain centre view
    (Resize(256, bicubic) + CenterCrop, bitwise ``tta.make_tta_views``' view 0), the rest are RandomResizedCrop(scale) + flip
    + AugMix(severity, width).  Records and recipe are ``group_records(..., seed)`` and ``sample_recipes(..., seed,
    plain=mask)``.  One ``augmix_batch`` call for every 65 536 views."""
    indices = [int(i) for i in indices]
    G, V = len(indices), 1 + int(n_views)
    if G == 0 or n_views < 0:
        raise ValueError(f"view_groups: {G} images, {n_views} views")
    recs, plain = group_records(pool, indices, n_views, scale=scale, size=size, seed=seed)
    recipe = sample_recipes(G * V, size, width=width, severity=severity, seed=seed, plain=plain)
    if out is None:
        out = torch.empty(G, V, 3, size, size, device=pool.device, dtype=torch.float32)
    elif tuple(out.shape) != (G, V, 3, size, size) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"view_groups: out must be a contiguous fp32 [{G}, {V}, 3, {size}, {size}] tensor")
    flat = out.view(G * V, 3, size, size)
    for lo in range(0, G * V, MAX_VIEWS):
        hi = min(lo + MAX_VIEWS, G * V)
        augmix_batch(pool, recs[lo:hi], Recipe(*(t[lo:hi] for t in recipe)), size, out=flat[lo:hi])
    return out
