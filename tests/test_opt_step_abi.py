"""Gradient clipping, the EMA shadow and the extended AdamW without a GPU: every new entry point refuses bad arguments
before launching anything, the work-size query is a host function, and the trainers validate the new arguments by
value before they touch a model."""
import math
import os
import re

import pytest

STATE = 0x10000  # never dereferenced: every call below carries one argument that is refused first
CLIP = 0x18000
BUF = 0x20000
WORK = 0x30000
SHADOW = 0x40000

HYPER = (2e-4, 0.9, 0.999, 1e-8, 1e-2, 1.0)  # lr, beta1, beta2, eps, weight_decay, grad_scale


def _lib():
    from clipfs import _lib
    return _lib.load()


def _refused(lib, rc, word):
    assert rc == 1, rc  # CLIPFS_EINVAL
    assert word in lib.clipfs_last_error(), lib.clipfs_last_error()


def test_work_size_query():
    lib = _lib()
    q = lib.clipfs_grad_sumsq_work_doubles
    assert q(0) == 0
    assert q(1) == 1
    sizes = [1, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 8192, 8193, 370688, 370689, 2 ** 21 - 1, 2 ** 21, 2 ** 21 + 1,
             3934208, 2 ** 24, 2 ** 31 + 5, 2 ** 40]
    got = [q(n) for n in sizes]
    assert all(a <= b for a, b in zip(got, got[1:])), got  # monotone in n
    assert all(1 <= g <= 512 for g in got), got           # one lane adds them: bounded
    assert q(4096) == 1 and q(4097) == 2
    # dense check over the range where the run length changes from fixed to growing
    prev = 0
    for n in range(1, 3 * 2 ** 20, 4093):
        cur = q(n)
        assert cur >= prev
        prev = cur


def test_grad_sumsq_refusals():
    lib = _lib()
    _refused(lib, lib.clipfs_grad_sumsq(None, 8, WORK, None), b"gradient pointer")
    _refused(lib, lib.clipfs_grad_sumsq(BUF + 2, 8, WORK, None), b"gradient pointer")  # not a float address
    _refused(lib, lib.clipfs_grad_sumsq(BUF, 8, None, None), b"work buffer")
    _refused(lib, lib.clipfs_grad_sumsq(BUF, 8, WORK + 4, None), b"work buffer")       # not a double address
    _refused(lib, lib.clipfs_grad_sumsq(BUF, 0, WORK, None), b"n = 0")


def test_clip_decide_refusals():
    lib = _lib()
    _refused(lib, lib.clipfs_clip_decide(WORK, 8, 1.0, None, None, None), b"clip state")
    _refused(lib, lib.clipfs_clip_decide(WORK, 8, 1.0, None, CLIP + 4, None), b"clip state")
    _refused(lib, lib.clipfs_clip_decide(WORK, 8, 1.0, STATE + 8, CLIP, None), b"scaler state")
    _refused(lib, lib.clipfs_clip_decide(None, 8, 1.0, None, CLIP, None), b"work buffer")
    _refused(lib, lib.clipfs_clip_decide(WORK + 4, 8, 1.0, STATE, CLIP, None), b"work buffer")
    _refused(lib, lib.clipfs_clip_decide(WORK, 0, 1.0, None, CLIP, None), b"n = 0")
    for bad in (0.0, -1.0, math.inf, -math.inf, math.nan, 1e39):  # 1e39 is infinite as an fp32 number
        _refused(lib, lib.clipfs_clip_decide(WORK, 8, bad, None, CLIP, None), b"max_norm")


def test_adamw_ext_refusals():
    lib = _lib()
    f = lib.clipfs_adamw_ext
    _refused(lib, f(None, BUF, BUF, BUF, 8, 1, *HYPER, None, None, None, 0.0, None), b"pointer")
    _refused(lib, f(BUF, None, BUF, BUF, 8, 1, *HYPER, None, None, None, 0.0, None), b"pointer")
    _refused(lib, f(BUF, BUF, None, BUF, 8, 1, *HYPER, None, None, None, 0.0, None), b"pointer")
    _refused(lib, f(BUF, BUF, BUF, None, 8, 1, *HYPER, None, None, None, 0.0, None), b"pointer")
    _refused(lib, f(BUF, BUF + 1, BUF, BUF, 8, 1, *HYPER, None, None, None, 0.0, None), b"pointer")
    _refused(lib, f(BUF, BUF, BUF, BUF, 8, 1, *HYPER, STATE + 4, None, None, 0.0, None), b"scaler state")
    _refused(lib, f(BUF, BUF, BUF, BUF, 8, 1, *HYPER, None, CLIP + 8, None, 0.0, None), b"clip state")
    _refused(lib, f(BUF, BUF, BUF, BUF, 8, 1, *HYPER, None, None, SHADOW + 2, 0.999, None), b"ema shadow")
    _refused(lib, f(BUF, BUF, BUF, BUF, 8, 1, *HYPER, None, None, BUF, 0.999, None), b"ema shadow")  # aliases p
    for bad in (0.0, 1.0, -0.5, 1.5, math.nan, math.inf):
        _refused(lib, f(BUF, BUF, BUF, BUF, 8, 1, *HYPER, None, None, SHADOW, bad, None), b"ema_decay")
    _refused(lib, f(BUF, BUF, BUF, BUF, 0, 1, *HYPER, None, None, None, 0.0, None), b"n = 0")
    _refused(lib, f(BUF, BUF, BUF, BUF, 8, 0, *HYPER, None, None, None, 0.0, None), b"step")


def test_clip_record_layout_matches_the_header():
    """The word indices of clipfs/_lib.py are the CLIPFS_CLIP_* of include/clipfs.h, and the ABI is still version 2."""
    from clipfs import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "clipfs.h")).read()
    header = {k: int(v) for k, v in re.findall(r"#define CLIPFS_CLIP_([A-Z0-9_]+) (\d+)", src)}
    assert header == {"NORM": 0, "COEF": 1, "MULT": 2, "WORDS": 8}
    assert header == {k: getattr(_lib, "CLIP_" + k) for k in header}
    assert int(re.search(r"#define CLIPFS_ABI_VERSION (\d+)", src).group(1)) == 2 == _lib.ABI_VERSION
    for name in ("clipfs_grad_sumsq_work_doubles", "clipfs_grad_sumsq", "clipfs_clip_decide", "clipfs_adamw_ext"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)


BAD_OPTIONS = [
    dict(max_grad_norm=0.0), dict(max_grad_norm=-1.0), dict(max_grad_norm=float("inf")), dict(max_grad_norm=float("nan")),
    dict(max_grad_norm=1e39), dict(max_grad_norm="1"), dict(max_grad_norm=True),
    dict(ema_decay=0.0), dict(ema_decay=1.0), dict(ema_decay=-0.1), dict(ema_decay=1.5), dict(ema_decay=float("nan")),
    dict(ema_decay=1.0 - 1e-12), dict(ema_decay="0.999"), dict(ema_decay=True)]


@pytest.mark.parametrize("kw", BAD_OPTIONS)
def test_lora_trainer_rejects_bad_options(kw):
    """Refused by value, before the model is looked at (none is needed to get here)."""
    import lora_train_vlp as L
    with pytest.raises(ValueError, match=next(iter(kw))):
        L.LoRATrainer(None, **kw)


@pytest.mark.parametrize("kw", BAD_OPTIONS)
def test_fused_stage2_trainer_rejects_bad_options(kw):
    import slow_pace as S
    with pytest.raises(ValueError, match=next(iter(kw))):
        S.Stage2Trainer(None, None, None, None, None, fused=True, **kw)


@pytest.mark.parametrize("kw", [dict(max_grad_norm=1.0), dict(ema_decay=0.999)])
def test_unfused_stage2_trainer_refuses_the_options(kw):
    """With the wording it uses for loss_scale: they belong to the fused step."""
    import slow_pace as S
    with pytest.raises(ValueError, match="belong to the fused step"):
        S.Stage2Trainer(None, None, None, None, None, **kw)
    with pytest.raises(ValueError, match=next(iter(kw))):
        S.Stage2Trainer(None, None, None, None, None, **kw)
