"""Replays every tower entry point of two versions of csrc/tower.hip against LOGGING STUBS of the kernel wrappers, without a
GPU, and compares what they would have enqueued: a check for host-side refactors of the sequencer.

    python scripts/replay_tower.py [--against REV]        (default REV: HEAD, i.e. the working tree against the last commit)

Both versions are compiled with stand-ins for every launching clipfs_* function tower.hip calls (generated from
include/clipfs.h), for clipfs_gemm_nt (which logs its argument struct byte by byte) and for hipMemcpyAsync /
hipMemsetAsync; the pure host queries (workspace sizes, *_ok predicates) come from the built libclipfs_hip.so.  A driver
then calls the seven entry points over a matrix of descriptors with fake addresses (geometries, storage formats, ranks,
dropout, adapter masks, frozen adapters, bias slots, deep prompts, gradient floor, stop_at_input, saving or not), once
plainly and once under CLIPFS_DENSE_BWD=1.  Equal logs = the same wrapper calls in the same order with the same
arguments, and the same return codes and *_mode / size answers.  Descriptors are complete, so checks that only one
version makes do not show."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "jittor-clip-fewshot_amd")
TOWER = "jittor-clip-fewshot_amd/csrc/tower.hip"
LIB = os.path.join(PKG, "clipfs", "libclipfs_hip.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"), "-I",
         os.path.join(PKG, "csrc"), "-Wno-unused-function", "-ffp-contract=off"]


def write_stubs(path):
    hdr = open(os.path.join(ROOT, "include", "clipfs.h")).read()
    hdr_nc = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    hdr_nc = re.sub(r"//[^\n]*", "", hdr_nc)
    names = """clipfs_add_seq_rows clipfs_attention_bwd clipfs_attention_bwd_packed clipfs_attention_bwd_packed_io clipfs_attention_f16_bwd
    clipfs_attention_f16_fwd clipfs_attention_fwd clipfs_attention_fwd_packed clipfs_bias_grad clipfs_convert_f16 clipfs_gather_rows_map
    clipfs_gather_seq_rows clipfs_gather_seq_rows_f16 clipfs_layernorm_bwd clipfs_layernorm_bwd_f16 clipfs_layernorm_bwd_rows
    clipfs_layernorm_fwd clipfs_layernorm_fwd_f16 clipfs_layernorm_fwd_lora clipfs_layernorm_fwd_lora_map clipfs_lora_bwd clipfs_lora_bwd_f16dy
    clipfs_lora_down clipfs_prompt_harvest clipfs_prompt_put clipfs_put_rows_map clipfs_put_seq_rows clipfs_put_seq_rows_f16
    clipfs_scatter_rows""".split()
    out = ['#include "common.h"', '#include <sstream>', '#include <string.h>', 'extern "C" {',
           'static FILE* lg() { static FILE* f = fopen(getenv("REPLAY_LOG"), "a"); return f; }',
           '}',
           'template <class T> static void put1(std::ostringstream& o, T v) { o << " " << v; }',
           'static void put1(std::ostringstream& o, float v) { char b[40]; snprintf(b, 40, " %a", v); o << b; }',
           'template <class... A> static int logcall(const char* n, A... a) { std::ostringstream o; o << n; (put1(o, a), ...); fprintf(lg(), "%s\\n", o.str().c_str()); fflush(lg()); return 0; }',
           'extern "C" {']
    for n in names:
        m = re.search(r'(?:CLIPFS_API\s+)?int\s+' + n + r'\s*\(([^;]*?)\)\s*;', hdr_nc, flags=re.S)
        assert m, n
        params = [p.strip() for p in m.group(1).replace('\n', ' ').split(',')]
        pn = [re.search(r'(\w+)\s*$', p).group(1) for p in params]
        cast = []
        for p, q in zip(params, pn):
            cast.append(f'(const void*){q}' if '*' in p else q)
        out.append(f'int {n}({", ".join(params)}) {{ return logcall("{n}", {", ".join(cast)}); }}')
    out.append('''int clipfs_gemm_nt(const clipfs_gemm_args* a, void* st) {
      std::ostringstream o; o << "clipfs_gemm_nt";
      const unsigned char* b = (const unsigned char*)a; char h[4];
      for (size_t i = 0; i < sizeof(*a); ++i) { snprintf(h, 4, "%02x", b[i]); if (i % 8 == 0) o << " "; o << h; }
      fprintf(lg(), "%s st=%p\\n", o.str().c_str(), st); fflush(lg()); return 0; }
    hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind k, hipStream_t st) { logcall("hipMemcpyAsync", (const void*)d, s, n, (int)k, (const void*)st); return hipSuccess; }
    hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t st) { logcall("hipMemsetAsync", (const void*)d, v, n, (const void*)st); return hipSuccess; }
    }''')
    open(path, "w").write("\n".join(out) + "\n")


def build(workdir, tag, tower_src):
    obj = os.path.join(workdir, f"tower_{tag}.o")
    subprocess.run([HIPCC, *FLAGS, "-c", tower_src, "-o", obj], check=True)
    so = os.path.join(workdir, f"libreplay_{tag}.so")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,-Bsymbolic", "-o", so, obj,
                    os.path.join(workdir, "stubs.o"), LIB, "-Wl,-rpath," + os.path.dirname(LIB)], check=True)
    return so


def drive(libpath, log):
    """(child process) calls every entry point of ``libpath`` over the descriptor matrix; the stubs append to ``log``"""
    sys.path.insert(0, PKG)
    from clipfs import _lib as L
    os.environ["REPLAY_LOG"] = log
    open(log, "w").close()
    C.CDLL(LIB, mode=C.RTLD_GLOBAL)
    lib = C.CDLL(libpath)
    for n in ["clipfs_tower_fwd", "clipfs_tower_fwd_rows", "clipfs_tower_fwd_packed", "clipfs_tower_bwd",
              "clipfs_tower_bwd_sparse", "clipfs_tower_bwd_packed", "clipfs_tower_bwd_packed_saved", "clipfs_tower_pack_mode",
              "clipfs_tower_pack_fwd_mode", "clipfs_tower_rows_mode", "clipfs_tower_saved_floats",
              "clipfs_tower_scratch_floats", "clipfs_tower_counter_ints"]:
        getattr(lib, n).restype, getattr(lib, n).argtypes = L.SIGNATURES[n]
    PTR = [0x10000000]
    def fake():
        PTR[0] += 0x1000000
        return PTR[0]

    def tower(layers, width, seq, causal, r, p, seed, wf, grad_lo, masks, frozen, bias, prompts, counters):
        PTR[0] = 0x10000000
        t = L.new_tower()
        blocks = (L.Block * layers)()
        for i, b in enumerate(blocks):
            for n, _ in L.Block._fields_:
                if n in ('lora_mask', 'prompt_first', 'prompt_rows'): continue
                setattr(b, n, fake())
            b.lora_mask = masks[i % len(masks)]
            if r == 0:
                b.lora_a_qkv = b.lora_b_qkv = b.lora_a_o = b.lora_b_o = None
            if r == 0 or i < grad_lo or (frozen and i % 2 == 0):
                b.g_lora_a_qkv = b.g_lora_b_qkv = None
            if r == 0 or i < grad_lo or (frozen and i % 2 == 1):
                b.g_lora_a_o = b.g_lora_b_o = None
            if b.lora_mask & 8 == 0: b.lora_a_o = b.lora_b_o = b.g_lora_a_o = b.g_lora_b_o = None
            if not bias or wf == 2 or i < grad_lo:
                for n in ("g_ln1_b", "g_ln2_b", "g_b_q", "g_b_k", "g_b_v", "g_b_o", "g_b_fc", "g_b_pr"): setattr(b, n, None)
            elif bias == 2:  # some only
                for n in ("g_ln2_b", "g_b_k", "g_b_o", "g_b_pr"): setattr(b, n, None)
            if prompts and i in prompts:
                b.prompt_first, b.prompt_rows = 1, 4
                if i < grad_lo or prompts[i] == 0: b.g_prompt = None
            else:
                b.prompt = b.g_prompt = None
        t.blocks = C.cast(blocks, C.POINTER(L.Block)); t._keep = blocks
        t.width, t.heads, t.layers, t.seq, t.causal = width, width // 64, layers, seq, causal
        t.lora_r, t.lora_scale, t.lora_dropout, t.dropout_seed = r, 0.5, p, seed
        t.dropout_stream0, t.dropout_row0 = 11, 1000
        t.weight_format, t.grad_lo = wf, grad_lo
        if counters:
            t.gemm_counters, t.gemm_counters_ints = fake(), 1 << 20
        return t

    def note(s):
        with open(log, 'a') as f: f.write(s + '\n')

    X, ROWS, PLAN, SAVED, SCR, DXS, DX = (0x7000000000 + i * 0x100000000 for i in range(7))
    ncase = 0
    def run(desc, t, batch, R):
        nonlocal ncase
        tp = C.byref(t)
        note(f'## {desc} batch={batch} R={R} modes rows={lib.clipfs_tower_rows_mode(tp)} pack={lib.clipfs_tower_pack_mode(tp, batch, R)} '
             f'packfwd={lib.clipfs_tower_pack_fwd_mode(tp, batch, R)} saved={lib.clipfs_tower_saved_floats(tp, batch)} '
             f'scratch={lib.clipfs_tower_scratch_floats(tp, batch)} cnt={lib.clipfs_tower_counter_ints(tp, batch)}')
        calls = []
        for saved in (SAVED, None):
            calls += [('fwd', lambda s=saved: lib.clipfs_tower_fwd(tp, X, batch, s, SCR, None)),
                      ('fwd_rows', lambda s=saved: lib.clipfs_tower_fwd_rows(tp, X, ROWS, batch, s, SCR, None)),
                      ('fwd_packed', lambda s=saved: lib.clipfs_tower_fwd_packed(tp, X, ROWS, PLAN, R, batch, s, SCR, None))]
        for stop in (1, 0):
            calls += [('bwd', lambda s=stop: lib.clipfs_tower_bwd(tp, DX, batch, SAVED, SCR, s, None)),
                      ('bwd_sparse', lambda s=stop: lib.clipfs_tower_bwd_sparse(tp, DXS, ROWS, DX, batch, SAVED, SCR, s, None)),
                      ('bwd_packed', lambda s=stop: lib.clipfs_tower_bwd_packed(tp, DXS, ROWS, PLAN, R, DX, batch, SAVED, SCR, s, None)),
                      ('bwd_packed_saved', lambda s=stop: lib.clipfs_tower_bwd_packed_saved(tp, DXS, ROWS, PLAN, R, DX, batch, SAVED, SCR, s, None))]
        for i, (name, fn) in enumerate(calls):
            note(f'# {name} #{i}')
            rc = fn()
            note(f'rc={rc}' + ('' if rc == 0 else ' ERR'))
            ncase += 1

    geoms = [  # layers, width, seq, causal, batch, R
        (3, 512, 77, 1, 403, 9748), (3, 512, 77, 1, 51, 1300), (2, 512, 77, 1, 10, 200), (3, 768, 50, 0, 32, 0), (2, 1024, 257, 0, 4, 0),
        (2, 768, 77, 1, 40, 1500), (2, 64, 77, 1, 40, 200), (2, 512, 120, 1, 30, 900), (1, 512, 77, 1, 403, 9748), (2, 192, 12, 1, 6, 30),
        (2, 512, 300, 0, 8, 0), (2, 512, 6, 1, 400, 900)]
    for (layers, width, seq, causal, batch, R) in geoms:
        if R == 0: R = batch
        for wf in (0, 1, 2):
            for (r, p, seed) in ((0, 0.0, 0), (4, 0.25, 7), (4, 0.25, 0), (4, 0.0, 7), (8, 0.25, 7), (16, 0.25, 7), (32, 0.25, 7), (64, 0.0, 7)):
                if r > 16 and width % 128: continue
                for masks in ((7,), (15,), (15, 7), (0, 7, 8), (5, 15, 7)):
                    if r == 0 and masks != (7,): continue
                    for grad_lo in (0, 1):
                        if grad_lo >= layers: continue
                        for frozen, bias, prompts in ((0, 0, None), (1, 1, {0: 1, layers - 1: 0}), (0, 2, {grad_lo: 1}), (1, 0, {layers - 1: 1})):
                            t = tower(layers, width, seq, causal, r, p, seed, wf, grad_lo, masks, frozen, bias, prompts, counters=(r % 8 == 0))
                            run(f'L{layers} w{width} s{seq} c{causal} wf{wf} r{r} p{p} seed{seed} m{masks} lo{grad_lo} fz{frozen} bias{bias} pr{prompts}', t, batch, R)
    print(f"{os.path.basename(libpath)}: {ncase} calls replayed", flush=True)


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--drive":
        return drive(sys.argv[2], sys.argv[3])
    rev = sys.argv[sys.argv.index("--against") + 1] if "--against" in sys.argv else "HEAD"
    if not os.path.isfile(LIB):
        raise SystemExit("build the library first (python jittor-clip-fewshot_amd/build.py)")
    with tempfile.TemporaryDirectory() as wd:
        old = os.path.join(wd, "tower_ref.hip")
        with open(old, "wb") as f:
            f.write(subprocess.run(["git", "-C", ROOT, "show", f"{rev}:{TOWER}"], check=True, capture_output=True).stdout)
        write_stubs(os.path.join(wd, "stubs.hip"))
        subprocess.run([HIPCC, *FLAGS, "-c", os.path.join(wd, "stubs.hip"), "-o", os.path.join(wd, "stubs.o")], check=True)
        libs = {"ref": build(wd, "ref", old), "tree": build(wd, "tree", os.path.join(ROOT, TOWER))}
        same = True
        for knob in ("0", "1"):
            logs = {}
            for tag, so in libs.items():
                logs[tag] = os.path.join(wd, f"{tag}_{knob}.log")
                subprocess.run([sys.executable, os.path.abspath(__file__), "--drive", so, logs[tag]], check=True,
                               env=dict(os.environ, CLIPFS_DENSE_BWD=knob))
            a, b = open(logs["ref"]).read(), open(logs["tree"]).read()
            print(f"CLIPFS_DENSE_BWD={knob}: {a.count(chr(10))} log lines, {'identical' if a == b else 'DIFFERENT'}")
            if a != b:
                same = False
                la, lb = a.split("\n"), b.split("\n")
                i = next(i for i in range(min(len(la), len(lb))) if la[i] != lb[i])
                head = max(j for j in range(i + 1) if la[j].startswith("## "))
                print("first difference in case:", la[head], "\n  ref :", la[i][:300], "\n  tree:", lb[i][:300])
        raise SystemExit(0 if same else 1)


if __name__ == "__main__":
    main()
