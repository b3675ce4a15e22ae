"""clipfs_gemm_f16_plan without a GPU: the kernel ids and the plan struct of clipfs/_lib.py are those of include/clipfs.h,
the ABI version stays 2 (a new entry point and new types: no existing field or parameter moves), and the query neither
launches nor follows a pointer."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "clipfs.h")).read()


def test_kernel_ids_match_the_header():
    from clipfs import _lib
    ids = {name: int(v) for name, v in re.findall(r"#define CLIPFS_F16_([A-Z0-9_]+) (\d+)", _header())}
    assert sorted(ids.values()) == list(range(9))
    assert [k for k, _ in sorted(ids.items(), key=lambda kv: kv[1])] == [n.upper() for n in _lib.F16_KERNELS]


def test_plan_struct_matches_the_header():
    from clipfs import _lib
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    launch = re.search(r"typedef struct clipfs_f16_launch \{(.*?)\} clipfs_f16_launch;", src, flags=re.S).group(1)
    plan = re.search(r"typedef struct clipfs_f16_plan \{(.*?)\} clipfs_f16_plan;", src, flags=re.S).group(1)
    names = lambda body: [n.strip() for decl in re.findall(r"int ([^;]+);", body) for n in decl.split(",")]
    assert names(launch) == [n for n, _ in _lib.F16Launch._fields_] and all(t is C.c_int for _, t in _lib.F16Launch._fields_)
    assert names(plan) == ["n"] and re.search(r"clipfs_f16_launch launch\[3\];", plan)
    assert [n for n, _ in _lib.F16Plan._fields_] == ["n", "launch"]
    assert C.sizeof(_lib.F16Launch) == 16 and C.sizeof(_lib.F16Plan) == 4 + 3 * 16


def test_abi_version_is_unchanged():
    from clipfs import _lib
    assert "#define CLIPFS_ABI_VERSION 2" in _header()
    assert _lib.load().clipfs_abi_version() == _lib.ABI_VERSION == 2


def test_query_follows_no_pointer_and_fills_unused_slots_with_zero():
    """Every pointer is an address nobody mapped (and odd ones at that where validation lets them be)."""
    from clipfs import _lib
    lib = _lib.load()
    g = _lib.new_gemm_args()
    g.M, g.N, g.K, g.lda, g.ldb, g.ldc, g.ldres = 2088, 2560, 128, 128, 128, 2560, 2560
    g.alpha = 1.0
    g.A_f16, g.B_planes, g.b_format = 0x10, 0x20, 2
    g.C, g.C_f16, g.bias, g.residual = 0x34, 0x42, 0x54, 0x64
    g.lora_t, g.lora_b, g.lora_r, g.lora_nseg, g.lora_seg_width = 0x71, 0x81, 8, 1, 2560
    out = _lib.F16Plan()
    for l in out.launch:
        l.kernel = l.m_begin = l.m_end = l.side = -1
    assert lib.clipfs_gemm_f16_plan(C.byref(g), 256, C.byref(out)) == 0, lib.clipfs_last_error()
    got = [(l.kernel, l.m_begin, l.m_end, l.side) for l in out.launch]
    assert out.n == 2 and got == [(4, 0, 2048, 0), (1, 2048, 2088, 1), (0, 0, 0, 0)]
    assert _lib.gemm_f16_plan(g, 256) == [("pp_reg", 0, 2048, False), ("64x128_s2", 2048, 2088, True)]
