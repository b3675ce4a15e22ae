"""The f16 x f16 GEMM (clipfs_gemm_nt with A_f16: csrc/gemm_f16.hip) over every kernel x epilogue family x leading
dimension, against the ONE fp64 restatement of the epilogue (gemm_matrix_helpers.ref_gemm) on the f16-rounded operands,
adapter operands rounded the way the kernel rounds them.  Same method as test_gemm_matrix_gpu.py: the entry point is driven
through ctypes so that the test owns every pointer.

  * layouts: tight; padded and aligned (lda = ldb = K + 8, ldc = N + 16, ldres = N + 24); padded so that only the
    register epilogue can store the rows (ldc = N + 13, ldres = N + 21); C, bias or the residual 4 bytes off 16-byte
    alignment;
  * sentinels: every output (fp32 C, f16 C, fp32 / f16 aux_out), the guard rows behind it and the guard words around it
    hold a NaN of the element's own type before the call; so do the padding columns of every input and the guard rows
    behind A, B, the residual, aux_in and the adapter operands.  After the call everything outside [M, N] of an output
    and every input buffer is compared bitwise;
  * every case (gemm_f16_cases.GPU_CASES / AID_CASES) first asserts, through clipfs_gemm_f16_plan on the device's CU count,
    that the dispatch sends it to the kernels, row ranges and stream it is there for (pytest.fail with the plan, no skip);
    then (b) results within budget, (c) guards and padding untouched, (d) a second call gives equal bits.

Budgets, those of test_gemm_f16_operands / test_gemm_f16_lds_epilogue_modes, with scale = max |reference| of the tensor:
  fp32 outputs (C, fp32 aux_out):  max |got - want| <= 2e-5 * scale + 1e-5;
  f16 outputs (C_f16, f16 aux_out): per element |got - want| <= 2^-11 |want| + (2e-5 * scale + 1e-5): one rounding of an
  fp32-accurate value.
Every case prints its errors before it asserts.  Worst seen on an MI355X over the 296 cases and the 39 under an aid:
  fp32 outputs 2.0e-6 against a budget of 1.2e-4 (2303 x 2568 x 448, rank-64 adapter, 32x32x16 phased kernel + leftovers);
  f16 outputs 3.8e-7 beyond the element's own rounding against 1.1e-4 (2303 x 2568 x 448, f16-only result, wide epilogue).
No case came near a budget: the only defect found is alpha != 1 together with an adapter (5.2e-1 and 6.5e-1 against
6e-5 at 257 x 403 x 96 and 2088 x 2560 x 128 with the refusal compiled out), now refused by the entry point.
Duration on an MI355X: 300 tests in 27 s, 15 s of them the five child processes (interpreter and device start-up).

Stream ordering: twenty rounds of (copy one of two A images, GEMM, copy C out) on a non-default stream without a host
synchronisation; every round's C must be that of its image, leftover rows (side stream) included.
Cached tuning aids (CLIPFS_F16_PHASED / _EPILOGUE / _SIDE / _TILE): one fresh child process per aid, sequentially."""
import ctypes as C
import subprocess
from collections import OrderedDict

import pytest
import torch

import gemm_f16_cases as cases
from gemm_f16_cases import AID_CASES, EPI, GPU_CASES, LORA_SCALE, gemm_args, leading_dims, lora_seg_width
from gemm_matrix_helpers import _bits, _nan_f16, _nan_f32, _sent_of, ref_gemm

pytestmark = pytest.mark.gpu

GUARD_ROWS = 3
HEAD = 8                   # guard elements in front of and behind every buffer (a multiple of 16 bytes in both types)
F16_EPS = 2.0 ** -11


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


# ------------------------------------------------------------------ inputs and fp64 products, once per (K, size class)
class Master:
    """Seeded operands of the largest shape of a class; every case of the class takes leading rows of them, so the fp64
    product is computed once per K."""

    def __init__(self, dev, Mx, Nx, K):
        g = torch.Generator().manual_seed(1000003 * Mx + 1009 * Nx + K)
        rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
        self.dev, self.Mx, self.Nx, self.K = dev, Mx, Nx, K
        self.a16 = rnd(Mx, K).half()
        self.b16 = (rnd(Nx, K) * K ** -0.5).half()
        self.acc = self.a16.double() @ self.b16.double().t()
        self.bias = rnd(Nx)
        self.res = rnd(Mx, Nx)
        self.aux = rnd(Mx, Nx).half()                      # the saved pre-activation: the same values as f16 and as fp32
        assert (self.aux > 0).any() and (self.aux < 0).any()
        self.lora = {}
        self.on_dev = {}

    def lora_of(self, r, nseg):
        if (r, nseg) not in self.lora:
            g = torch.Generator().manual_seed(77 * r + nseg)
            self.lora[(r, nseg)] = (torch.randn(self.Mx, nseg * r, generator=g), torch.randn(self.Nx, r, generator=g) * 0.1)
        return self.lora[(r, nseg)]

    def d(self, name):
        if name not in self.on_dev:
            self.on_dev[name] = getattr(self, name).to(self.dev)
        return self.on_dev[name]


_MASTERS = OrderedDict()


def master_for(dev, M, N, K):
    if M <= 257 and N <= 403:
        key = (257, 403, K)
    elif 2048 <= M <= 2303 and N <= 2568:
        key = (2303, 2568, K)
    elif N == 2048:
        key = (8488, 2048, K)
    else:
        key = (M, N, K)
    if key not in _MASTERS:
        while len(_MASTERS) >= 2:  # cases arrive grouped by class: keep the memory of two
            _MASTERS.popitem(last=False)
        _MASTERS[key] = Master(dev, *key)
    return _MASTERS[key]


# ------------------------------------------------------------------ guarded buffers
class Buf:
    """[rows, ld] of `dtype` filled with the NaN sentinel, HEAD guard elements in front and behind; `off` elements (of 4
    bytes) move the matrix off its 16-byte alignment."""

    def __init__(self, dev, rows, ld, dtype, off=0):
        fill = _nan_f16 if dtype == torch.float16 else _nan_f32
        start = HEAD + off
        self.flat = fill(start + rows * ld + HEAD, dev=dev)
        self.mat = self.flat[start:start + rows * ld].view(rows, ld)
        assert self.flat.data_ptr() % 16 == 0 and self.ptr % 16 == (4 * off if off else 0)

    @property
    def ptr(self):
        return self.mat.data_ptr()

    def put(self, x):
        self.mat[:x.shape[0], :x.shape[1]] = x
        return self

    def outside_untouched(self, M, N):
        """(ok, first offender) over everything but [M, N]"""
        bits = _bits(self.flat).clone()
        start = self.mat.data_ptr() - self.flat.data_ptr()
        start //= self.flat.element_size()
        bits[start:start + self.mat.numel()].view(self.mat.shape)[:M, :N] = _sent_of(self.flat)
        bad = (bits != _sent_of(self.flat)).nonzero()
        return bad.numel() == 0, (bad[0].item() - start if bad.numel() else None, bad.shape[0])


def _stream_ptr(stream=None):
    return (torch.cuda.current_stream() if stream is None else stream).cuda_stream


def setup_case(dev, c):
    """Device buffers and the argument block of one case: (args, inputs {name: Buf}, outputs {name: Buf})"""
    e = EPI[c.epi]
    M, N, K = c.M, c.N, c.K
    m = master_for(dev, M, N, K)
    lda, ldb, ldc, ldres = leading_dims(c.layout, N, K)
    off = lambda name: 1 if c.offset == name else 0
    ins, outs, ptr = {}, {}, {}
    ins["A16"] = Buf(dev, M + GUARD_ROWS, lda, torch.float16).put(m.d("a16")[:M])
    ins["B16"] = Buf(dev, N + GUARD_ROWS, ldb, torch.float16).put(m.d("b16")[:N])
    if e["out"] in ("c32", "both"):
        outs["C"] = Buf(dev, M + GUARD_ROWS, ldc, torch.float32, off("C"))
    if e["out"] in ("c16", "both"):
        outs["C16"] = Buf(dev, M + GUARD_ROWS, ldc, torch.float16)
    if e["bias"]:
        ins["bias"] = Buf(dev, 1, N, torch.float32, off("bias")).put(m.d("bias")[None, :N])
    if e["residual"]:
        ins["residual"] = Buf(dev, M + GUARD_ROWS, ldres, torch.float32, off("residual")).put(m.d("res")[:M, :N])
    if e["aux"]:
        dt = torch.float16 if e["aux"] == "f16" else torch.float32
        if e["act"] == 1:
            outs["aux"] = Buf(dev, M + GUARD_ROWS, ldc, dt)
        else:
            ins["aux"] = Buf(dev, M + GUARD_ROWS, ldc, dt).put(m.d("aux")[:M, :N].to(dt))
    if e["lora"]:
        r, nseg, _ = e["lora"]
        t, lb = m.lora_of(r, nseg)
        ins["lora_t"] = Buf(dev, M + GUARD_ROWS, nseg * r, torch.float32).put(t[:M].to(dev))
        ins["lora_b"] = Buf(dev, N + GUARD_ROWS, r, torch.float32).put(lb[:N].to(dev))
    for name, b in list(ins.items()) + list(outs.items()):
        ptr[name] = b.ptr
    for name in cases.POINTERS:
        ptr.setdefault(name, 0)
    return gemm_args(M, N, K, c.layout, e, ptr), ins, outs


def reference(dev, c):
    """{output name: fp64 reference on the device}"""
    e = EPI[c.epi]
    M, N = c.M, c.N
    m = master_for(dev, M, N, c.K)
    lora = None
    if e["lora"]:
        r, nseg, kind = e["lora"]
        t, lb = m.lora_of(r, nseg)
        lora = (t[:M].double(), lb[:N].double(), lora_seg_width(N, nseg, kind), LORA_SCALE)
    want, pre = ref_gemm(None, None, acc=m.acc[:M, :N], alpha=e["alpha"], bias=m.bias[:N].double() if e["bias"] else None,
                         lora=lora, lora_f16=True, act=e["act"], aux_in=m.aux[:M, :N].double() if e["act"] == 2 else None,
                         residual=m.res[:M, :N].double() if e["residual"] else None)
    ref = {}
    if e["out"] in ("c32", "both"):
        ref["C"] = want
    if e["out"] in ("c16", "both"):
        ref["C16"] = want
    if e["act"] == 1 and e["aux"]:
        ref["aux"] = pre
    return {k: v.to(dev) for k, v in ref.items()}


def call(lib, g, stream=None):
    return lib.clipfs_gemm_nt(C.byref(g), _stream_ptr(stream))


def measure(got, want):
    """(error, budget): fp32 tensors max |got - want| against 2e-5 scale + 1e-5; f16 tensors the worst excess of an element
    over its own rounding 2^-11 |want| against the same budget.  NaN (never written, or computed from padding) is infinite."""
    budget = 2e-5 * want.abs().max().item() + 1e-5
    d = (got.double() - want).abs()
    if got.dtype == torch.float16:
        d = d - F16_EPS * want.abs()
    return (float("inf") if torch.isnan(d).any() else d.max().item()), budget


def check_plan(lib, c, g):
    from clipfs import _lib
    plan = tuple(_lib.gemm_f16_plan(g, 0))
    if plan != c.plan:
        pytest.fail(f"{c.name}: the dispatch plans {plan} on this device, the case is there for {c.plan}")


def check_case(dev, c, tag="gemm-f16"):
    """(a) - (d) of the module docstring for one case; returns {output: (error, budget)}"""
    from clipfs import _lib
    lib = _lib.load()
    g, ins, outs = setup_case(dev, c)
    check_plan(lib, c, g)                                                   # (a)
    before = {k: _bits(b.flat).clone() for k, b in ins.items()}
    rc = call(lib, g)
    assert rc == 0, (rc, lib.clipfs_last_error())
    torch.cuda.synchronize()
    ref = reference(dev, c)
    assert sorted(ref) == sorted(outs)
    res = {k: measure(outs[k].mat[:c.M, :c.N], ref[k]) for k in sorted(outs)}
    print(f"[{tag}] {c.name}: " + "  ".join(f"{k}({'f16' if outs[k].flat.dtype == torch.float16 else 'fp32'}) err {e:.3e} "
                                            f"budget {b:.3e} ratio {e / b:.3f}" for k, (e, b) in res.items()))
    for k, (e, b) in res.items():                                           # (b)
        assert e <= b, f"{c.name} {k}: error {e:.3e} > budget {b:.3e}"
    for k, b in outs.items():                                               # (c)
        ok, where = b.outside_untouched(c.M, c.N)
        assert ok, f"{c.name} {k}: {where[1]} elements outside [M, N] written, first at element {where[0]} of the matrix"
    for k, b in ins.items():
        assert torch.equal(_bits(b.flat), before[k]), f"{c.name}: input {k} changed"
    g2, ins2, outs2 = setup_case(dev, c)                                    # (d)
    assert call(lib, g2) == 0
    torch.cuda.synchronize()
    for k in outs:
        assert torch.equal(_bits(outs[k].flat), _bits(outs2[k].flat)), f"{c.name} {k}: a second call gives other bits"
    return res


@pytest.mark.parametrize("c", GPU_CASES, ids=[c.name for c in GPU_CASES])
def test_f16_gemm_case(dev, c):
    check_case(dev, c)


# ------------------------------------------------------------------ alpha != 1 with an adapter is refused
@pytest.mark.parametrize("shape", [(257, 403, 96), (2088, 2560, 128)], ids=["4wave", "phased"])
def test_alpha_with_adapter_is_refused(dev, shape):
    """The adapter product is accumulated by MFMA steps into the accumulator that alpha then scales, so alpha != 1 would
    scale it too, against the order include/clipfs.h states.  No caller combines the two (csrc/tower.hip passes alpha 1,
    clipfs/engine.py passes alpha without an adapter): the entry point refuses, naming both, and writes nothing."""
    from clipfs import _lib
    lib = _lib.load()
    c = cases.Case("refused", *shape, "aligned", "alpha_lora16", None, None, ())
    g, ins, outs = setup_case(dev, c)
    assert call(lib, g) == 1
    msg = lib.clipfs_last_error()
    assert b"alpha" in msg and b"lora_t" in msg, msg
    torch.cuda.synchronize()
    for k, b in outs.items():
        assert bool((_bits(b.flat) == _sent_of(b.flat)).all().item()), k
    g.alpha = 1.0   # the same arguments with alpha 1 run
    assert call(lib, g) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(outs["C"].mat[:c.M, :c.N]).any()


# ------------------------------------------------------------------ fork and join of the side stream
def test_side_stream_is_ordered_with_the_callers_stream(dev):
    from clipfs import _lib
    lib = _lib.load()
    c = next(x for x in GPU_CASES if (x.M, x.N, x.K, x.layout, x.epi) == (2088, 2560, 128, "tight", "plain"))
    assert c.plan == (("ph16", 0, 2048, False), ("64x128_s2", 2048, 2088, True))
    g, ins, outs = setup_case(dev, c)
    check_plan(lib, c, g)
    a_buf, c_buf = ins["A16"].flat, outs["C"].flat
    images = [a_buf.clone(), a_buf.clone()]
    images[1][HEAD:HEAD + c.M * c.K] = torch.flip(images[0][HEAD:HEAD + c.M * c.K].view(c.M, c.K), dims=(0,)).reshape(-1)
    want = []
    for img in images:                                   # what each image gives, synchronously
        a_buf.copy_(img)
        c_buf.copy_(_nan_f32(c_buf.numel(), dev=dev))
        assert call(lib, g) == 0
        torch.cuda.synchronize()
        want.append(c_buf.clone())
    assert not torch.equal(want[0][HEAD:HEAD + 64 * c.N], want[1][HEAD:HEAD + 64 * c.N])
    assert not torch.equal(want[0].view(torch.int32)[HEAD + 2048 * c.N:HEAD + c.M * c.N],
                           want[1].view(torch.int32)[HEAD + 2048 * c.N:HEAD + c.M * c.N]), "leftover rows must differ too"
    pattern = [0, 1, 1, 0, 1, 0, 0, 1, 0, 1, 1, 1, 0, 0, 1, 0, 1, 0, 0, 1]
    got = [torch.empty_like(c_buf) for _ in pattern]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for i, which in enumerate(pattern):              # no host synchronisation in here
            a_buf.copy_(images[which], non_blocking=True)
            rc = call(lib, g, s)
            got[i].copy_(c_buf, non_blocking=True)
            assert rc == 0
    s.synchronize()
    for i, which in enumerate(pattern):
        same = got[i].view(torch.int32) == want[which].view(torch.int32)
        if not bool(same.all().item()):
            first = (~same).nonzero()[0].item() - HEAD
            pytest.fail(f"round {i} (image {which}): C differs from that image's result, first at row {first // c.N}")


# ------------------------------------------------------------------ cached tuning aids: one child process each
def child_main(aid):
    """child side: the cases of AID_CASES[aid]; the plan check inside check_case proves that the aid is in force"""
    dev = torch.device("cuda:0")
    for c in AID_CASES[aid]:
        assert c.env == aid
        check_case(dev, c, tag=f"gemm-f16 {aid}")
    print("CHILD OK")


def test_cached_aids_in_child_processes(dev):
    for aid in AID_CASES:
        cmd = cases.child_command(f"import test_gemm_f16_matrix_gpu as t; t.child_main({aid!r})")
        r = subprocess.run(cmd, env=cases.child_env(aid), capture_output=True, text=True, timeout=180)
        print(r.stdout)
        assert r.returncode == 0 and "CHILD OK" in r.stdout, f"{aid}: exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
