"""A poisoning allocator for the workspace-independence tests (test_workspace_*_gpu.py).

Inside ``poisoned(fill)`` every uninitialised floating-point device allocation the package makes is filled with ``fill``
before it is returned, so a kernel that reads a slot before writing it, or multiplies a masked 0 by a stale row, computes
a different (or non-finite) result than under another fill.  The tests run the same call under 0.0, NaN and 1e30 and
compare the outputs bit for bit.

Patched calls (every uninitialised-allocation call in use in the package):

    torch.empty          ops.py, engine.py, resnet.py, data.py, dist.py, views.py, lora_train_vlp.py, slow_pace.py,
                         ood.py, tpt.py
    torch.empty_like     ops.py, engine.py
    torch.Tensor.new_empty   not in use today; patched so that a first use cannot slip past these tests

found with

    grep -rnoE "(torch\\.empty\\w*|\\bempty_like|\\.new_empty\\w*|empty_strided|\\.new\\(|resize_|\\.set_\\()" \\
        jittor-clip-fewshot_amd --include="*.py"

(no empty_strided, Tensor.new, resize_ or set_ in the package; every hit is ``torch.empty(`` or ``torch.empty_like(``,
called through the ``torch`` module attribute, which is what gets patched).

Only floating-point CUDA tensors (fp32, f16, bf16) are filled.  Integer, bool and CPU tensors pass through untouched ON
PURPOSE: a poisoned index table could send a kernel to a wild address, and these tests must only ever be able to produce
wrong values, never a GPU fault.  Keep it that way.
"""
import contextlib
import math

import torch

FILLS = (0.0, float("nan"), 1.0e30)
FILL_IDS = ("zero", "nan", "1e30")
_FLOAT = (torch.float32, torch.float16, torch.bfloat16)


def fill_value(dtype, fill):
    """``fill`` as representable in ``dtype``: 1e30 overflows f16, whose largest finite value stands in for it."""
    if dtype == torch.float16 and math.isfinite(fill) and abs(fill) > 65504.0:
        return math.copysign(65504.0, fill)
    return fill


def poison_(t, fill):
    """Fill ``t`` in place on the current stream when it is a floating-point device tensor; returns ``t``."""
    if isinstance(t, torch.Tensor) and t.is_cuda and t.dtype in _FLOAT and t.numel():
        t.fill_(fill_value(t.dtype, fill))
    return t


@contextlib.contextmanager
def poisoned(fill):
    """Patch the allocation calls listed in the module docstring for the duration of the block."""
    real_empty, real_like, real_new = torch.empty, torch.empty_like, torch.Tensor.new_empty

    def empty(*args, **kw):
        return poison_(real_empty(*args, **kw), fill)

    def empty_like(*args, **kw):
        return poison_(real_like(*args, **kw), fill)

    def new_empty(self, *args, **kw):
        return poison_(real_new(self, *args, **kw), fill)

    torch.empty, torch.empty_like, torch.Tensor.new_empty = empty, empty_like, new_empty
    try:
        yield
    finally:
        torch.empty, torch.empty_like, torch.Tensor.new_empty = real_empty, real_like, real_new


@contextlib.contextmanager
def poisoned_towers(fill, counters_seen=None):
    """``poisoned(fill)`` plus the per-tower buffers of ``clipfs.engine._TowerRT.buffer``, which are handed out again
    step after step: "scratch" is refilled on every request (every forward and backward asks for it), "saved" only when
    ``forward`` asks (the backward receives it as an argument and must find the forward's data).  The ("counters", 0)
    tensor does not come from ``buffer`` and is never filled: it is an index-like table the GEMMs must leave zero.
    Every request also asserts that the tower's counters are all zero: a tower call asks for its scratch first, so this
    is the state the previous call of that tower left behind (the caller checks the last one: ``counters_zero``).
    ``counters_seen``: a list that receives every tower runtime that asked for a buffer, for that last check."""
    import sys

    from clipfs import engine
    real = engine._TowerRT.buffer

    def buffer(self, kind, n_floats, device):
        buf = real(self, kind, n_floats, device)
        assert counters_zero(self), f"{self.name} tower: split-K counters not zero after a tower call"
        if counters_seen is not None and not any(rt is self for rt in counters_seen):
            counters_seen.append(self)
        if kind == "scratch" or (kind == "saved" and sys._getframe(1).f_code.co_name == "forward"):
            poison_(buf, fill)
        return buf

    engine._TowerRT.buffer = buffer
    try:
        with poisoned(fill):
            yield
    finally:
        engine._TowerRT.buffer = real


def counters_zero(rt):
    """Whether the split-K arrival counters of tower runtime ``rt`` are all zero (True when it has none)."""
    buf = rt._bufs.get(("counters", 0))
    return buf is None or not bool(buf.any().item())


def same_bits(a, b):
    """torch.equal on the raw bits: NaN equals the same NaN, and nothing passes because nan != nan."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.is_floating_point:
        view = {4: torch.int32, 2: torch.int16, 8: torch.int64}[a.element_size()]
        a, b = a.contiguous().view(view), b.contiguous().view(view)
    return torch.equal(a, b)


def all_finite(t):
    return bool(torch.isfinite(t).all().item())


def assert_same_runs(runs, ids=FILL_IDS):
    """``runs``: one dict of named output tensors per fill, in the order of FILLS.  Every floating-point output is finite
    and every output is bitwise equal across the fills."""
    torch.cuda.synchronize()
    first = runs[0]
    for name, t in first.items():
        if t.dtype.is_floating_point:
            assert all_finite(t), f"{name}: non-finite under fill {ids[0]}"
    for k, run in enumerate(runs[1:], 1):
        assert run.keys() == first.keys(), (sorted(run), sorted(first))
        for name, t in run.items():
            assert same_bits(t, first[name]), f"{name}: fill {ids[k]} differs from fill {ids[0]}"
