"""Every entry point of include/clipfs.h that takes caller scratch, and the poison test that exercises it.

``TABLE[name] = (size query, GPU test)``: the size query is the header function (or plan field) that sizes the scratch
parameter; the test is ``<module>::<function>`` under tests/, which runs the entry point with that memory pre-filled
with 0.0, NaN and 1e30 and compares the outputs bit for bit (tests/poison.py).  ``EXEMPT[name]`` gives the one-line
reason why an entry point with such a parameter needs no row.  tests/test_workspace_table.py parses the header and fails
when a function with a scratch parameter is in neither, so the next kernel cannot slip past the poison tests.

A scratch parameter is one named in SCRATCH_NAMES, or a pointer to a struct that has such a member
(clipfs_gemm_args.workspace)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "clipfs.h")

# work / scratch / workspace / saved by name; loss_rows is the cross entropy's documented scratch (a D-buffer-like temporary)
SCRATCH_NAMES = ("work", "scratch", "workspace", "saved", "loss_rows")

K = "test_workspace_kernels_gpu"
T = "test_workspace_towers_gpu"

TABLE = {
    # attention: work = D_i = dO_i . O_i, as long as lse
    "clipfs_attention_bwd": ("clipfs_attention_lse_floats", f"{K}::test_attention_fp32"),
    "clipfs_attention_f16_bwd": ("clipfs_attention_lse_floats", f"{K}::test_attention_f16"),
    "clipfs_attention_f16_bwd_packed": ("clipfs_attention_lse_floats", f"{K}::test_attention_f16_packed"),
    # adapters
    "clipfs_lora_bwd": ("clipfs_lora_bwd_work_floats", f"{K}::test_lora"),
    "clipfs_lora_bwd_xact": ("clipfs_lora_bwd_work_floats2", f"{K}::test_lora"),
    "clipfs_lora_bwd_f16dy": ("clipfs_lora_bwd_work_floats", f"{K}::test_lora"),
    # smaller kernels
    "clipfs_bias_grad": ("clipfs_bias_grad_work_floats", f"{K}::test_bias_grad"),
    "clipfs_mta": ("clipfs_mta_work_floats", f"{K}::test_mta"),
    "clipfs_tpt_objective": ("clipfs_tpt_work_floats", f"{K}::test_tpt_objective"),
    "clipfs_grad_sumsq": ("clipfs_grad_sumsq_work_doubles", f"{K}::test_grad_sumsq_clip_decide"),
    "clipfs_clip_decide": ("clipfs_grad_sumsq_work_doubles", f"{K}::test_grad_sumsq_clip_decide"),
    "clipfs_cross_entropy": ("2 * rows", f"{K}::test_cross_entropy"),
    "clipfs_cross_entropy_scaled": ("2 * rows", f"{K}::test_cross_entropy"),
    "clipfs_stage2_objective": ("4 * B + C_loc", f"{T}::test_stage2_fused_step"),
    # tower drivers
    "clipfs_tower_fwd": ("clipfs_tower_scratch_floats, clipfs_tower_saved_floats", f"{T}::test_sequencer_dense_and_sparse"),
    "clipfs_tower_bwd": ("clipfs_tower_scratch_floats, clipfs_tower_saved_floats", f"{T}::test_sequencer_dense_and_sparse"),
    "clipfs_tower_fwd_rows": ("clipfs_tower_scratch_floats, clipfs_tower_saved_floats", f"{T}::test_sequencer_dense_and_sparse"),
    "clipfs_tower_bwd_sparse": ("clipfs_tower_scratch_floats, clipfs_tower_saved_floats", f"{T}::test_sequencer_dense_and_sparse"),
    "clipfs_tower_bwd_packed": ("clipfs_tower_scratch_floats, clipfs_tower_saved_floats", f"{T}::test_packed_text_paths"),
    "clipfs_tower_fwd_packed": ("clipfs_tower_scratch_floats, clipfs_tower_saved_floats", f"{T}::test_packed_text_paths"),
    "clipfs_tower_bwd_packed_saved": ("clipfs_tower_scratch_floats, clipfs_tower_saved_floats", f"{T}::test_packed_text_paths"),
}

EXEMPT = {
    "clipfs_gemm_nt": "split-K workspace and every matrix carry sentinels in tests/test_gemm_matrix_gpu.py",
    "clipfs_gemm_plan": "host-only: no pointer of the descriptor is dereferenced",
    "clipfs_gemm_f16_plan": "host-only: no pointer of the descriptor is dereferenced",
    "clipfs_attention_mfma_long_bwd": "the kernels clipfs_attention_bwd launches past 288 tokens (test_attention_fp32 at 289); "
                                      "its explicit cuts are bitwise that call in tests/test_attention_fp32_long_gpu.py",
    "clipfs_logit_normalize": "work holds two floats, written by the first launch before the second reads them; "
                              "fp64 parity in tests/test_kernels_gpu.py",
    "clipfs_kl_logits": "loss_rows is a documented output here, not scratch",
    "clipfs_contrastive_objective": "work behind NaN guards in tests/test_contrastive_gpu.py; loss_rows is an output",
}

# Outputs the header documents as (partly) unwritten: the poison tests leave them out of the comparison, or assert that
# the region keeps its fill.  Listed so that a reader of a failing comparison knows what is deliberately not compared.
DOCUMENTED_UNINITIALISED = {
    "clipfs_tower_bwd": "dx with stop_at_input != 0 (the gradient wrt the tower input is not formed)",
    "clipfs_tower_bwd_sparse": "dx with stop_at_input != 0",
    "clipfs_tower_bwd_packed": "dx with stop_at_input != 0",
    "clipfs_tower_bwd_packed_saved": "dx with stop_at_input != 0",
    "clipfs_tower_fwd_rows": "x outside the rows c * seq + rows[c] keeps the last block's input",
    "clipfs_tower_fwd_packed": "x outside the rows c * seq + rows[c] is unspecified",
    "clipfs_attention_fwd_packed": "lse entries past Lb are left unwritten (asserted: they keep their fill)",
}

_PROTO = re.compile(r"^(?:int|size_t|long|double|void\s*\*|const\s+char\s*\*|void)\s*\**\s*(clipfs_\w+)\s*\(([^;{}]*?)\)\s*;", re.M | re.S)
_STRUCT = re.compile(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", re.S)


def _strip_comments(text):
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def _param_name(param):
    m = re.search(r"(\w+)\s*(?:\[\s*\d*\s*\])?\s*$", param.strip())
    return m.group(1) if m else ""


def scratch_structs(text):
    """Names of the typedef'd structs of the header that have a member named like scratch."""
    out = set()
    for m in _STRUCT.finditer(_strip_comments(text)):
        members = [_param_name(f) for f in m.group(2).split(";") if f.strip()]
        if any(n in SCRATCH_NAMES for n in members):
            out.update((m.group(1), m.group(3)))
    return out


def prototypes(text):
    """{function name: [parameter declarations]} of every ``clipfs_*`` prototype of the header text."""
    out = {}
    for m in _PROTO.finditer(_strip_comments(text)):
        params = [p.strip() for p in m.group(2).replace("\n", " ").split(",")]
        out[m.group(1)] = [p for p in params if p and p != "void"]
    return out


def scratch_functions(text):
    """{function name: [its scratch parameters]} for the header text."""
    structs = scratch_structs(text)
    out = {}
    for name, params in prototypes(text).items():
        hits = [p for p in params if _param_name(p) in SCRATCH_NAMES and "*" in p]
        hits += [p for p in params if any(re.search(rf"\b{s}\s*\*", p) for s in structs)]
        if hits:
            out[name] = hits
    return out


def read_header():
    with open(HEADER) as f:
        return f.read()
