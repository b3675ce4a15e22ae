"""ctypes binding of libclipfs_hip.so (C ABI in include/clipfs.h).

The library is the only compute path of this package: if it is missing the
import fails loudly -- there is NO PyTorch / CPU fallback.  Build it with
``python jittor-clip-fewshot_amd/build.py`` (or ``__graft_entry__.build()``).
"""
from __future__ import annotations

import ctypes as C
import os

ABI_VERSION = 2  # CLIPFS_ABI_VERSION of include/clipfs.h this table was written against

_HERE = os.path.dirname(os.path.abspath(__file__))
# CLIPFS_LIB_TAG=<tag>: an experiment build made with `build.py --tag <tag>` (A/B timing of kernel variants in one
# gpurun call; bench.py lists it among the active overrides).  Unset = the product library.
_TAG = os.environ.get("CLIPFS_LIB_TAG", "")
LIB_PATH = os.path.join(_HERE, f"libclipfs_hip_{_TAG}.so" if _TAG else "libclipfs_hip.so")

c_f32p = C.c_void_p  # device pointers travel as integers (tensor.data_ptr())
c_stream = C.c_void_p


class ClipfsError(RuntimeError):
    pass


class GemmArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_size_t),
        ("A", C.c_void_p), ("B", C.c_void_p), ("C", C.c_void_p),
        ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
        ("lda", C.c_int), ("ldb", C.c_int), ("ldc", C.c_int),
        ("alpha", C.c_float),
        ("bias", C.c_void_p), ("residual", C.c_void_p), ("ldres", C.c_int),
        ("act", C.c_int), ("aux_out", C.c_void_p), ("aux_in", C.c_void_p),
        ("lora_t", C.c_void_p), ("lora_b", C.c_void_p),
        ("lora_r", C.c_int), ("lora_nseg", C.c_int), ("lora_seg_width", C.c_int),
        ("lora_scale", C.c_float),
        ("a_mode", C.c_int), ("img_res", C.c_int), ("patch", C.c_int), ("out_tokens", C.c_int),
        ("B_planes", C.c_void_p), ("b_format", C.c_int), ("workspace", C.c_void_p), ("workspace_floats", C.c_size_t),
        ("A_f16", C.c_void_p), ("C_f16", C.c_void_p), ("aux_f16", C.c_int),
        ("counters", C.c_void_p), ("counters_ints", C.c_size_t),
    ]


class F16Launch(C.Structure):
    _fields_ = [("kernel", C.c_int), ("m_begin", C.c_int), ("m_end", C.c_int), ("side", C.c_int)]


class F16Plan(C.Structure):
    _fields_ = [("n", C.c_int), ("launch", F16Launch * 3)]


class GemmPlan(C.Structure):
    _fields_ = [("kernel", C.c_int), ("planes", C.c_int), ("tile_rows", C.c_int), ("splits", C.c_int), ("want_splits", C.c_int),
                ("mix_rows64", C.c_int), ("gm", C.c_int), ("grid", C.c_int), ("block", C.c_int), ("lds_bytes", C.c_int),
                ("workspace_floats", C.c_size_t), ("counter_ints", C.c_size_t)]


class AttentionLaunch(C.Structure):
    _fields_ = [("grid_x", C.c_uint), ("grid_y", C.c_uint), ("block", C.c_uint), ("lds_bytes", C.c_uint)]


class AttentionPlan(C.Structure):
    _fields_ = [("family", C.c_int), ("nt", C.c_int), ("parts", C.c_int), ("tiles", C.c_int), ("ctok", C.c_int),
                ("lmax", C.c_int), ("launches", C.c_int), ("launch", AttentionLaunch * 2)]


# CLIPFS_ATTN_* directions, flags and kernel families of include/clipfs.h, by value
ATTN_DIRECTIONS = ("fwd", "bwd", "fwd_packed", "bwd_packed", "bwd_packed_io")
ATTN_STATS, ATTN_ALIGNED = 1, 2
ATTN_FAMILIES = ("mfma16", "mfma16_packed", "mfma16_pinned", "mfma32", "mfma_long", "stream", "recompute",
                 "f16_short", "f16_long")  # the first seven: what clipfs_attention_plan returns; the last two: the f16 plan
ATTN_F16_DIRECTIONS = ("fwd", "bwd", "bwd_packed")

class LoraLaunch(C.Structure):
    _fields_ = [("grid_x", C.c_uint), ("grid_y", C.c_uint), ("block", C.c_uint)]


class LoraPlan(C.Structure):
    _fields_ = [("family", C.c_int), ("groups", C.c_int), ("rq", C.c_int), ("sr_b", C.c_int), ("slices_b", C.c_int),
                ("sr_a", C.c_int), ("slices_a", C.c_int), ("work_floats", C.c_size_t), ("part_a_offset", C.c_size_t),
                ("keep_bits_ok", C.c_int), ("f16dy_ok", C.c_int), ("launches", C.c_int), ("launch", LoraLaunch * 6)]


# CLIPFS_LORA_* operations, flags and kernel families of include/clipfs.h, by value
LORA_OPS = ("down", "bwd", "bwd_f16dy")
LORA_X_ACT, LORA_KEEP_BITS, LORA_FROZEN, LORA_DX = 1, 2, 4, 8
LORA_FAMILIES = ("mfma", "row")

# CLIPFS_F16_* kernel ids of include/clipfs.h, by value
F16_KERNELS = ("64x128", "64x128_s2", "128x128", "256x128", "pp_reg", "pp_lds", "ph16", "ph16_wide", "ph32")
# CLIPFS_GEMM_* kernel ids of include/clipfs.h, by value
GEMM_KERNELS = ("nt64", "nt64_reg", "nt32", "mixed", "patch32", "generic", "planes64", "planes128")


class CachePlan(C.Structure):
    """struct clipfs_cache_plan: what a cache-head entry point launches."""
    _fields_ = [("grid_x", C.c_uint), ("grid_y", C.c_uint), ("grid_z", C.c_uint), ("block", C.c_uint), ("lds_bytes", C.c_uint),
                ("class_chunk", C.c_int), ("feat_chunk", C.c_int), ("beta_chunk", C.c_int), ("alpha_chunk", C.c_int), ("work_floats", C.c_size_t)]


# CLIPFS_CACHE_OP_* of include/clipfs.h, by value
CACHE_OPS = ("logits", "bwd_dk", "bwd_df", "search")


class ContrastivePlan(C.Structure):
    """struct clipfs_contrastive_plan: what clipfs_contrastive_objective launches."""
    _fields_ = [("grid_x", C.c_uint), ("grid_y", C.c_uint), ("grid_z", C.c_uint), ("block", C.c_uint), ("lds_bytes", C.c_uint),
                ("col_chunk", C.c_int), ("chunks", C.c_int), ("feat_chunk", C.c_int), ("work_floats", C.c_size_t)]


# CLIPFS_CONTRASTIVE_OP_* of include/clipfs.h, by value
CONTRASTIVE_OPS = ("stats", "combine", "dq", "dk")


class SigmoidPlan(C.Structure):
    """struct clipfs_sigmoid_plan: what clipfs_sigmoid_objective launches."""
    _fields_ = [("grid_x", C.c_uint), ("grid_y", C.c_uint), ("grid_z", C.c_uint), ("block", C.c_uint), ("lds_bytes", C.c_uint),
                ("feat_chunk", C.c_int)]


# CLIPFS_SIGMOID_OP_* of include/clipfs.h, by value
SIGMOID_OPS = ("rows", "combine", "dq", "dk")


class ClipPairsPlan(C.Structure):
    """struct clipfs_clip_pairs_plan: what clipfs_clip_pairs_objective launches."""
    _fields_ = [("grid_x", C.c_uint), ("grid_y", C.c_uint), ("grid_z", C.c_uint), ("block", C.c_uint), ("lds_bytes", C.c_uint),
                ("feat_chunk", C.c_int)]


# CLIPFS_PAIRS_OP_* of include/clipfs.h, by value
CLIP_PAIRS_OPS = ("rows", "combine", "dq", "dk")


class TdaParams(C.Structure):
    """struct clipfs_tda_params: the fixed inputs of the TDA rule."""
    _fields_ = [("struct_size", C.c_uint), ("C", C.c_int), ("d", C.c_int), ("pos_cap", C.c_int), ("neg_cap", C.c_int),
                ("logit_scale", C.c_float), ("pos_alpha", C.c_float), ("pos_beta", C.c_float), ("neg_alpha", C.c_float),
                ("neg_beta", C.c_float), ("ent_lo", C.c_float), ("ent_hi", C.c_float), ("mask_lo", C.c_float), ("mask_hi", C.c_float)]


TDA_STATE_FIELDS = ("pos_keys", "pos_ent", "pos_seq", "neg_keys", "neg_ent", "neg_seq", "neg_mask", "counter")
TDA_RECORD_FIELDS = ("pred", "entropy", "hnorm", "band", "seq", "mask", "pos_slot", "neg_slot", "pos_born", "pos_evict",
                     "neg_born", "neg_evict")


class TdaState(C.Structure):
    """struct clipfs_tda_state: device pointers of the two caches and the sample counter."""
    _fields_ = [("struct_size", C.c_uint)] + [(n, C.c_void_p) for n in TDA_STATE_FIELDS]


class TdaRecord(C.Structure):
    """struct clipfs_tda_record: device pointers of the per-sample outputs of clipfs_tda_adapt."""
    _fields_ = [("struct_size", C.c_uint)] + [(n, C.c_void_p) for n in TDA_RECORD_FIELDS]


class TdaLaunch(C.Structure):
    _fields_ = [("grid_x", C.c_uint), ("grid_y", C.c_uint), ("block", C.c_uint), ("lds_bytes", C.c_uint)]


# CLIPFS_TDA_LAUNCH_* of include/clipfs.h, by value
TDA_LAUNCHES = ("z", "stats", "scan", "logits", "write")


class TdaPlan(C.Structure):
    """struct clipfs_tda_plan: what clipfs_tda_adapt launches, and the sizes of its state and record."""
    _fields_ = [("launches", C.c_int), ("launch", TdaLaunch * 5), ("lds_bytes", C.c_uint), ("class_chunk", C.c_int),
                ("pos_entries", C.c_size_t), ("neg_entries", C.c_size_t), ("pos_key_floats", C.c_size_t),
                ("neg_key_floats", C.c_size_t), ("neg_mask_bytes", C.c_size_t), ("mask_bytes", C.c_size_t)]


class TransductParams(C.Structure):
    """struct clipfs_transduct_params: the shapes and hyper-parameters of a transductive fit."""
    _fields_ = [("struct_size", C.c_uint), ("N", C.c_int), ("C", C.c_int), ("d", C.c_int), ("M", C.c_int), ("k", C.c_int),
                ("init_top", C.c_int), ("outer", C.c_int), ("inner", C.c_int), ("knn_chunks", C.c_int),
                ("logit_scale", C.c_float), ("lam", C.c_float), ("shot_weight", C.c_float), ("n_min", C.c_float),
                ("var_floor", C.c_float)]


# members of struct clipfs_transduct_buffers, in order (shot_labels_host is host memory, the rest device memory)
TRANSDUCT_BUFFER_FIELDS = ("feats", "text", "shots", "shot_labels", "shot_labels_host", "z", "labels", "zs_labels", "mu", "var",
                           "nbr", "w", "logy", "u", "z2", "mup", "bias", "n", "G", "Q", "shot_n", "shot_G", "sel", "stat_work",
                           "knn_work")


class TransductBuffers(C.Structure):
    """struct clipfs_transduct_buffers: inputs, outputs, state and work of the transductive stages."""
    _fields_ = [("struct_size", C.c_uint)] + [(n, C.c_void_p) for n in TRANSDUCT_BUFFER_FIELDS]


class TransductLaunch(C.Structure):
    _fields_ = [("grid_x", C.c_uint), ("grid_y", C.c_uint), ("grid_z", C.c_uint), ("block", C.c_uint), ("lds_bytes", C.c_uint)]


# CLIPFS_TRANSDUCT_LAUNCH_* of include/clipfs.h, by value
TRANSDUCT_LAUNCHES = ("logits", "logsm", "knn", "knn_merge", "shots", "q", "init", "bias", "u", "z_step", "stats", "muvar")


class TransductPlan(C.Structure):
    """struct clipfs_transduct_plan: what a transductive fit launches, and the sizes of its work buffers."""
    _fields_ = [("launches", C.c_int), ("knn_chunks", C.c_int), ("class_chunk", C.c_int), ("stat_splits", C.c_int),
                ("stat_rows", C.c_int), ("launch", TransductLaunch * 12), ("lds_bytes", C.c_uint),
                ("knn_work_bytes", C.c_size_t), ("stat_work_floats", C.c_size_t), ("nc_floats", C.c_size_t)]


class SpdPlan(C.Structure):
    """struct clipfs_spd_plan: what clipfs_spd_factor and clipfs_spd_solve launch."""
    _fields_ = [("block", C.c_int), ("factor_launches", C.c_int), ("solve_launches", C.c_int), ("factor_grid", C.c_uint),
                ("solve_grid", C.c_uint), ("threads", C.c_uint), ("factor_lds_bytes", C.c_uint), ("solve_lds_bytes", C.c_uint),
                ("lds_bytes", C.c_uint)]


# CLIPFS_GDA_PRIOR_* of include/clipfs.h, by value
GDA_PRIORS = ("uniform", "empirical")


class GdaParams(C.Structure):
    """struct clipfs_gda_params: the shapes and hyper-parameters of a GDA fit."""
    _fields_ = [("struct_size", C.c_uint), ("M", C.c_int), ("C", C.c_int), ("d", C.c_int), ("prior", C.c_int),
                ("shrink", C.c_float)]


# members of struct clipfs_gda_buffers, in order (offsets_host is host memory, the rest device memory)
GDA_BUFFER_FIELDS = ("shots", "offsets", "offsets_host", "mu", "xt", "gram", "tau", "chol", "info", "W", "b")


class GdaBuffers(C.Structure):
    """struct clipfs_gda_buffers: the inputs and the named outputs of the GDA stages."""
    _fields_ = [("struct_size", C.c_uint)] + [(n, C.c_void_p) for n in GDA_BUFFER_FIELDS]


class GdaPlan(C.Structure):
    """struct clipfs_gda_plan: what a GDA fit launches."""
    _fields_ = [("launches", C.c_int), ("Mp", C.c_int), ("factor_launches", C.c_int), ("solve_launches", C.c_int),
                ("stats_grid", C.c_uint), ("bias_grid", C.c_uint), ("solve_grid", C.c_uint), ("threads", C.c_uint),
                ("lds_bytes", C.c_uint), ("xt_floats", C.c_size_t)]


class SpdPanelsPlan(C.Structure):
    """struct clipfs_spd_panels_plan: what clipfs_spd_factor_panels and clipfs_spd_solve_panels launch."""
    _fields_ = [("panel", C.c_int), ("panels", C.c_int), ("band", C.c_int), ("factor_launches", C.c_int),
                ("factor_gemms", C.c_int), ("solve_launches", C.c_int), ("solve_gemms", C.c_int), ("threads", C.c_uint),
                ("lds_bytes", C.c_uint)]


class KrrParams(C.Structure):
    """struct clipfs_krr_params: the shapes and hyper-parameters of a kernel ridge fit."""
    _fields_ = [("struct_size", C.c_uint), ("n", C.c_int), ("C", C.c_int), ("d", C.c_int), ("panel", C.c_int),
                ("beta", C.c_float), ("lambda_", C.c_float), ("t", C.c_float)]


class KrrBuffers(C.Structure):
    """struct clipfs_krr_buffers: the inputs and the named outputs of a kernel ridge fit (labels_host is host memory)."""
    _fields_ = [("struct_size", C.c_uint), ("shots", C.c_void_p), ("labels", C.c_void_p), ("labels_host", C.c_void_p),
                ("base_S", C.c_void_p), ("ldbs", C.c_int), ("A", C.c_void_p), ("chol", C.c_void_p), ("info", C.c_void_p),
                ("Et", C.c_void_p), ("At", C.c_void_p)]


class KrrPlan(C.Structure):
    """struct clipfs_krr_plan: what a kernel ridge fit and apply launch."""
    _fields_ = [("n4", C.c_int), ("panelled", C.c_int), ("fit_launches", C.c_int), ("factor_launches", C.c_int),
                ("solve_launches", C.c_int), ("tiles_per_wave", C.c_int), ("class_chunk", C.c_int), ("apply_grid_x", C.c_uint),
                ("apply_grid_y", C.c_uint), ("threads", C.c_uint), ("lds_bytes", C.c_uint)]


class OtPlan(C.Structure):
    """struct clipfs_ot_plan: what clipfs_ot_logits and clipfs_ot_bwd launch."""
    _fields_ = [("fwd_launches", C.c_int), ("dp_launches", C.c_int), ("dx_launches", C.c_int), ("rows_per_lane", C.c_int),
                ("prompt_regs", C.c_int), ("class_chunk", C.c_int), ("class_chunks", C.c_int), ("z_stride", C.c_int),
                ("dp_feat_chunk", C.c_int), ("dx_feat_chunk", C.c_int), ("fwd_grid", C.c_uint), ("dp_grid_x", C.c_uint),
                ("dp_grid_y", C.c_uint), ("dx_grid_x", C.c_uint), ("dx_grid_y", C.c_uint), ("threads", C.c_uint),
                ("fwd_lds_bytes", C.c_uint), ("bwd_lds_bytes", C.c_uint)]


class AugmixRecipe(C.Structure):
    """struct clipfs_augmix_recipe: host and device copies of the five recipe tables of clipfs_augmix_batch."""
    _fields_ = [("struct_size", C.c_uint)] + [(n + s, C.c_void_p) for n in ("ops", "coef", "depth", "w", "m") for s in ("", "_dev")]


class AugmixLaunch(C.Structure):
    _fields_ = [("grid_x", C.c_uint), ("grid_y", C.c_uint), ("block", C.c_uint), ("lds_bytes", C.c_uint)]


# CLIPFS_AUGMIX_LAUNCH_* and the operation codes CLIPFS_AUGMIX_* of include/clipfs.h, by value
AUGMIX_LAUNCHES = ("base", "chains", "mix")
AUGMIX_CODES = ("none", "autocontrast", "equalize", "posterize", "solarize", "affine")


class AugmixPlan(C.Structure):
    """struct clipfs_augmix_plan: what clipfs_augmix_batch launches, and the sizes of its two uint8 buffers."""
    _fields_ = [("launches", C.c_int), ("launch", AugmixLaunch * 3), ("lds_bytes", C.c_uint), ("base_bytes", C.c_size_t),
                ("chains_bytes", C.c_size_t), ("out_floats", C.c_size_t)]


class MergeJob(C.Structure):
    """struct clipfs_lora_merge_job: one projection of a clipfs_lora_merge table."""
    _fields_ = [("w", C.c_void_p), ("a", C.c_void_p), ("b", C.c_void_p), ("out", C.c_void_p), ("planes", C.c_void_p),
                ("n", C.c_int), ("k", C.c_int), ("nseg", C.c_int), ("seg_mask", C.c_uint), ("tile0", C.c_int),
                ("reserved", C.c_int)]


# CLIPFS_LORA_MERGE_TILE_ROWS / _COLS of include/clipfs.h
MERGE_TILE_ROWS, MERGE_TILE_COLS = 32, 256


def merge_job_tiles(n: int, k: int, nseg: int) -> int:
    """Tiles of one clipfs_lora_merge job (a tile never crosses a segment); the table's ``tile0`` is their prefix sum."""
    return nseg * (-(-(n // nseg) // MERGE_TILE_ROWS)) * (-(-k // MERGE_TILE_COLS))


class Block(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "ln1_g", "ln1_b", "ln2_g", "ln2_b",
        "w_qkv", "b_qkv", "w_qkv_t",
        "w_o", "b_o", "w_o_t",
        "w_fc", "b_fc", "w_fc_t",
        "w_pr", "b_pr", "w_pr_t",
        "lora_a_qkv", "lora_b_qkv", "lora_a_o", "lora_b_o",
        "g_lora_a_qkv", "g_lora_b_qkv", "g_lora_a_o", "g_lora_b_o")] + [("lora_mask", C.c_uint)] + [
        (n, C.c_void_p) for n in ("w_qkv_p", "w_o_p", "w_fc_p", "w_pr_p", "w_qkv_t_p", "w_o_t_p", "w_fc_t_p", "w_pr_t_p",
                                  "g_ln1_b", "g_ln2_b", "g_b_q", "g_b_k", "g_b_v", "g_b_o", "g_b_fc", "g_b_pr",
                                  "lora_a_fc", "lora_b_fc", "lora_a_pr", "lora_b_pr",
                                  "g_lora_a_fc", "g_lora_b_fc", "g_lora_a_pr", "g_lora_b_pr",
                                  "prompt", "g_prompt")] + [("prompt_first", C.c_int), ("prompt_rows", C.c_int)]


class Tower(C.Structure):
    _fields_ = [
        ("struct_size", C.c_size_t), ("block_size", C.c_size_t),
        ("width", C.c_int), ("heads", C.c_int), ("layers", C.c_int), ("seq", C.c_int), ("causal", C.c_int),
        ("lora_r", C.c_int), ("lora_scale", C.c_float), ("lora_dropout", C.c_float),
        ("dropout_seed", C.c_uint64), ("dropout_stream0", C.c_uint32), ("dropout_row0", C.c_uint32),
        ("blocks", C.POINTER(Block)), ("weight_format", C.c_int),
        ("gemm_counters", C.c_void_p), ("gemm_counters_ints", C.c_size_t),
        ("grad_lo", C.c_int),  # 0 = every block (today's behaviour)
    ]


_i, _f, _p, _sz = C.c_int, C.c_float, C.c_void_p, C.c_size_t
_u, _u64, _u32 = C.c_uint, C.c_uint64, C.c_uint32

# name -> (restype, argtypes).  Every symbol declared in include/clipfs.h is listed here and
# tests/test_abi.py checks the list against the header.
SIGNATURES = {
    "clipfs_abi_version": (_i, []),
    "clipfs_last_error": (C.c_char_p, []),
    "clipfs_source_stamp": (C.c_char_p, []),
    "clipfs_gemm_source_stamp": (C.c_char_p, []),
    "clipfs_gemm_nt": (_i, [C.POINTER(GemmArgs), _p]),
    "clipfs_split_bf16": (_i, [_p, _p, _sz, _p]),
    "clipfs_convert_f16": (_i, [_p, _p, _sz, _p]),
    "clipfs_gemm_plan": (_i, [C.POINTER(GemmArgs), C.POINTER(GemmPlan)]),
    "clipfs_gemm_splits": (_i, [_i, _i, _i]),
    "clipfs_gemm_tile_rows": (_i, [_i, _i]),
    "clipfs_gemm_mixed_rows64": (_i, [_i, _i, _i]),
    "clipfs_gemm_f16_plan": (_i, [C.POINTER(GemmArgs), _i, C.POINTER(F16Plan)]),
    "clipfs_gemm_workspace_floats": (_sz, [_i, _i, _i]),
    "clipfs_gemm_counter_ints": (_sz, [_i, _i, _i]),
    "clipfs_gemm_timing": (_i, [_i]),
    "clipfs_gemm_timing_collect": (_i, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "clipfs_gemm_timing_last_bytes": (C.c_double, []),
    "clipfs_layernorm_fwd": (_i, [_p, _i, _p, _p, _p, _p, _p, _i, _i, _f, _p]),
    "clipfs_layernorm_bwd": (_i, [_p, _p, _i, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "clipfs_layernorm_fwd_f16": (_i, [_p, _i, _p, _p, _p, _p, _p, _p, _i, _i, _f, _p]),
    "clipfs_layernorm_fwd_lora_ok": (_i, [_i, _i, _i]),
    "clipfs_layernorm_fwd_lora": (_i, [_p, _i, _p, _p, _p, _p, _p, _p, _i, _i, _f, _p, _p, _i, _i, _u, _f, _u64, _u32, _u32, _p, _p]),
    "clipfs_layernorm_bwd_f16": (_i, [_p, _p, _i, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "clipfs_attention_fwd": (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    "clipfs_attention_bwd": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "clipfs_attention_lse_floats": (_sz, [_i, _i, _i]),
    "clipfs_attention_plan": (_i, [_i, _i, _i, _i, _i, _i, C.POINTER(AttentionPlan)]),
    "clipfs_attention_mfma_max_seq": (_i, []),
    "clipfs_attention_mfma_long_fwd": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "clipfs_attention_mfma_long_bwd": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "clipfs_attention_f16_max_seq": (_i, []),
    "clipfs_attention_f16_plan": (_i, [_i, _i, _i, _i, _i, _i, C.POINTER(AttentionPlan)]),
    "clipfs_attention_f16_fwd": (_i, [_p, _i, _p, _p, _p, _i, _i, _i, _i, _p]),
    "clipfs_attention_f16_bwd": (_i, [_p, _i, _p, _i, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "clipfs_lora_keep_bits_ok": (_i, [_i, _i, _i, _i]),
    "clipfs_lora_plan": (_i, [_i, _i, _i, _i, _i, _i, _i, C.POINTER(LoraPlan)]),
    "clipfs_lora_down": (_i, [_p, _p, _p, _i, _i, _i, _i, _u, _f, _u64, _u32, _u32, _p, _p]),
    "clipfs_lora_bwd_work_floats": (_sz, [_i, _i, _i, _i]),
    "clipfs_lora_bwd": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _u, _f, _f, _u64, _u32, _u32, _p, _p, _p]),
    "clipfs_lora_bwd_work_floats2": (_sz, [_i, _i, _i, _i, _i]),
    "clipfs_lora_bwd_xact": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _f, _f, _u64, _u32, _u32, _i, _p, _p]),
    "clipfs_gelu_bwd_inplace": (_i, [_p, _p, _sz, _p]),
    "clipfs_lora_bwd_f16dy_ok": (_i, [_i, _i, _i, _i]),
    "clipfs_lora_bwd_f16dy": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _u, _f, _f, _u64, _u32, _u32, _p, _p, _p]),
    "clipfs_vit_fill_special": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "clipfs_text_embed": (_i, [_p, _p, _p, _p, _i, _p, _i, _i, _i, _p]),
    "clipfs_token_rows_grad": (_i, [_p, _p, _i, _i, _i, _i, _i, _p]),
    "clipfs_matmul_small": (_i, [_p, _p, _p, _i, _i, _i, C.c_long, C.c_long, C.c_long, C.c_long, _f, _p]),
    "clipfs_gather_eot": (_i, [_p, _p, _p, _p, _i, _i, _i, _p]),
    "clipfs_scatter_rows": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "clipfs_gather_seq_rows": (_i, [_p, _sz, _p, _p, _i, _i, _i, _p]),
    "clipfs_add_seq_rows": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "clipfs_put_seq_rows": (_i, [_p, _p, _p, _sz, _i, _i, _i, _p]),
    "clipfs_eot_index": (_i, [_p, _p, _i, _i, _p]),
    "clipfs_gather_seq_rows_f16": (_i, [_p, _sz, _p, _p, _i, _i, _i, _p]),
    "clipfs_put_seq_rows_f16": (_i, [_p, _p, _p, _sz, _i, _i, _i, _p]),
    "clipfs_l2norm_fwd": (_i, [_p, _p, _p, _i, _i, _p]),
    "clipfs_l2norm_bwd": (_i, [_p, _p, _p, _p, _i, _i, _p]),
    "clipfs_class_mean_fwd": (_i, [_p, _p, _i, _i, _i, _p]),
    "clipfs_class_mean_bwd": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "clipfs_cross_entropy": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _f, _p]),
    "clipfs_topk": (_i, [_p, _p, _i, _i, _i, _p]),
    "clipfs_channel_affine": (_i, [_p, _p, _p, _p, _i, _i, _p]),
    "clipfs_logit_normalize": (_i, [_p, _p, _p, _i, _i, _p]),
    "clipfs_logit_normalize_bwd": (_i, [_p, _p, _p, _i, _i, _p]),
    "clipfs_colsum": (_i, [_p, _p, _p, _i, _i, _p]),
    "clipfs_bias_grad_work_floats": (_sz, [_i, _i]),
    "clipfs_bias_grad": (_i, [_p, _sz, _i, _i, _i, _p, _p, _p, _p, _p]),
    "clipfs_l1_loss": (_i, [_p, _p, _sz, _p, _p, _f, _p]),
    "clipfs_kl_logits": (_i, [_p, _p, _p, _p, _i, _i, _f, _p]),
    "clipfs_stage2_objective": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _f, _p, _p]),
    "clipfs_adamw": (_i, [_p, _p, _p, _p, _sz, _i, _f, _f, _f, _f, _f, _f, _p]),
    "clipfs_cross_entropy_scaled": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _f, _p, _p]),
    "clipfs_grads_nonfinite": (_i, [_p, _sz, _p, _p]),
    "clipfs_scaler_decide": (_i, [_p, _f, _f, _f, _f, _f, _i, _p]),
    "clipfs_adamw_scaled": (_i, [_p, _p, _p, _p, _sz, _f, _f, _f, _f, _f, _p, _p]),
    "clipfs_grad_sumsq_work_doubles": (_sz, [_sz]),
    "clipfs_grad_sumsq": (_i, [_p, _sz, _p, _p]),
    "clipfs_clip_decide": (_i, [_p, _sz, _f, _p, _p, _p]),
    "clipfs_adamw_ext": (_i, [_p, _p, _p, _p, _sz, _i, _f, _f, _f, _f, _f, _f, _p, _p, _p, _f, _p]),
    "clipfs_adamw_tail": (_i, [_p, _p, _p, _p, _sz, _i, _f, _f, _f, _f, _f, _f, _p, _p, _p, _f, _sz, _f, _f, _f, _p]),
    "clipfs_mta_work_floats": (_sz, [_i, _i, _i, _i]),
    "clipfs_mta": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "clipfs_tta_views": (_i, [_p, _i, _i, _p, _i, _i, _p, _p, _p, _p]),
    "clipfs_crop_batch": (_i, [_p, _sz, _p, _p, _i, _p, _p, _i, _i, _p, _p, _p, _p, _p]),
    "clipfs_lora_merge": (_i, [C.POINTER(MergeJob), _p, _i, _sz, _i, _f, _i, _p]),
    "clipfs_bpe_create": (C.c_void_p, [C.c_char_p, _sz, _i]),
    "clipfs_bpe_destroy": (None, [C.c_void_p]),
    "clipfs_bpe_encode": (C.c_long, [C.c_void_p, _p, _p, _i, _p, _p, C.c_long]),
    "clipfs_nchw_to_nhwc": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "clipfs_im2col_nhwc": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "clipfs_maxpool3x3s2_nhwc": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "clipfs_global_avgpool_nhwc": (_i, [_p, _p, _i, _i, _i, _p]),
    "clipfs_avgpool_nhwc": (_i, [_p, _p, _i, _i, _i, _i, _i, _p]),
    "clipfs_attnpool_tokens": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "clipfs_attnpool_attend": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "clipfs_prompt_put": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "clipfs_prompt_harvest": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p, _p]),
    "clipfs_tower_saved_floats": (_sz, [C.POINTER(Tower), _i]),
    "clipfs_tower_scratch_floats": (_sz, [C.POINTER(Tower), _i]),
    "clipfs_tower_counter_ints": (_sz, [C.POINTER(Tower), _i]),
    "clipfs_tower_fwd": (_i, [C.POINTER(Tower), _p, _i, _p, _p, _p]),
    "clipfs_tower_fwd_rows": (_i, [C.POINTER(Tower), _p, _p, _i, _p, _p, _p]),
    "clipfs_tower_rows_mode": (_i, [C.POINTER(Tower)]),
    "clipfs_tower_bwd": (_i, [C.POINTER(Tower), _p, _i, _p, _p, _i, _p]),
    "clipfs_tower_bwd_sparse": (_i, [C.POINTER(Tower), _p, _p, _p, _i, _p, _p, _i, _p]),
    "clipfs_attention_bwd_packed_ok": (_i, [_i, _i]),
    "clipfs_attention_bwd_packed": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "clipfs_gather_rows_map": (_i, [_p, _sz, _p, _p, _i, _i, _p]),
    "clipfs_put_rows_map": (_i, [_p, _p, _p, _sz, _i, _i, _p]),
    "clipfs_layernorm_bwd_rows": (_i, [_p, _p, _i, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "clipfs_tower_pack_mode": (_i, [C.POINTER(Tower), _i, _i]),
    "clipfs_tower_bwd_packed": (_i, [C.POINTER(Tower), _p, _p, _p, _i, _p, _i, _p, _p, _i, _p]),
    "clipfs_layernorm_fwd_lora_map": (_i, [_p, _i, _p, _p, _p, _p, _p, _p, _i, _i, _f, _p, _p, _i, _i, _u, _f, _u64, _u32, _u32, _p,
                                           _p, _p]),
    "clipfs_attention_fwd_packed": (_i, [_p, _p, _p, _p, _i, _i, _i, _p]),
    "clipfs_attention_bwd_packed_io": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "clipfs_tower_pack_fwd_mode": (_i, [C.POINTER(Tower), _i, _i]),
    "clipfs_tower_fwd_packed": (_i, [C.POINTER(Tower), _p, _p, _p, _i, _i, _p, _p, _p]),
    "clipfs_tower_bwd_packed_saved": (_i, [C.POINTER(Tower), _p, _p, _p, _i, _p, _i, _p, _p, _i, _p]),
    "clipfs_attention_f16_bwd_packed_ok": (_i, [_i, _i]),
    "clipfs_attention_f16_bwd_packed": (_i, [_p, _i, _p, _i, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "clipfs_layernorm_bwd_rows_f16": (_i, [_p, _p, _i, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "clipfs_cache_plan": (_i, [_i, _i, _i, _i, _i, _i, _i, C.POINTER(CachePlan)]),
    "clipfs_cache_logits": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _f, _f, _p]),
    "clipfs_cache_bwd": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _f, _f, _p]),
    "clipfs_cache_search": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    "clipfs_tpt_work_floats": (_sz, [_i, _i, _i, _i]),
    "clipfs_tpt_objective": (_i, [_p, _p, _i, _p, _i, _i, _f, _f, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "clipfs_contrastive_plan": (_i, [_i, _i, _i, _i, C.POINTER(ContrastivePlan)]),
    "clipfs_contrastive_objective": (_i, [_p, _p, _p, _p, _f, _f, _p, _p, _p, _p, _p, _i, _p, _i, _p, _i, _i, _i, _p]),
    "clipfs_sigmoid_plan": (_i, [_i, _i, _i, _i, C.POINTER(SigmoidPlan)]),
    "clipfs_sigmoid_objective": (_i, [_p, _p, _p, _p, _p, _f, _p, _p, _p, _p, _p, _i, _p, _i, _p, _i, _i, _i, _i, _p]),
    "clipfs_clip_pairs_plan": (_i, [_i, _i, _i, _i, _i, C.POINTER(ClipPairsPlan)]),
    "clipfs_clip_pairs_objective": (_i, [_p, _p, _p, _p, _p, _f, _f, _p, _p, _p, _p, _p, _p, _i, _p, _i, _p, _i, _i, _i, _i, _p]),
    "clipfs_tda_plan": (_i, [C.POINTER(TdaParams), _i, _i, C.POINTER(TdaPlan)]),
    "clipfs_tda_adapt": (_i, [C.POINTER(TdaParams), _p, _p, C.POINTER(TdaState), _p, _i, C.POINTER(TdaRecord), _i, _i, _p]),
    "clipfs_transduct_plan": (_i, [C.POINTER(TransductParams), C.POINTER(TransductPlan)]),
    "clipfs_transduct_logy": (_i, [C.POINTER(TransductParams), C.POINTER(TransductBuffers), _p]),
    "clipfs_transduct_knn": (_i, [C.POINTER(TransductParams), C.POINTER(TransductBuffers), _p]),
    "clipfs_transduct_init": (_i, [C.POINTER(TransductParams), C.POINTER(TransductBuffers), _p]),
    "clipfs_transduct_u": (_i, [C.POINTER(TransductParams), C.POINTER(TransductBuffers), _p]),
    "clipfs_transduct_z_step": (_i, [C.POINTER(TransductParams), C.POINTER(TransductBuffers), _p, _p, _p, _p]),
    "clipfs_transduct_stats": (_i, [C.POINTER(TransductParams), C.POINTER(TransductBuffers), _p, _p]),
    "clipfs_transduct_fit": (_i, [C.POINTER(TransductParams), C.POINTER(TransductBuffers), _p]),
    "clipfs_spd_plan": (_i, [C.c_int, C.c_int, C.POINTER(SpdPlan)]),
    "clipfs_spd_factor": (_i, [_p, C.c_int, _p, C.c_int, C.c_int, _p, _p]),
    "clipfs_spd_solve": (_i, [_p, C.c_int, C.c_int, _p, C.c_int, _p, C.c_int, C.c_int, C.c_float, _p]),
    "clipfs_spd_panels_plan": (_i, [C.c_int, C.c_int, C.c_int, C.POINTER(SpdPanelsPlan)]),
    "clipfs_spd_factor_panels": (_i, [_p, C.c_int, _p, C.c_int, C.c_int, C.c_int, _p, _p]),
    "clipfs_spd_solve_panels": (_i, [_p, C.c_int, C.c_int, C.c_int, _p, C.c_int, _p, C.c_int, C.c_int, C.c_float, _p]),
    "clipfs_gda_plan": (_i, [C.POINTER(GdaParams), C.POINTER(GdaPlan)]),
    "clipfs_gda_stats": (_i, [C.POINTER(GdaParams), C.POINTER(GdaBuffers), _p]),
    "clipfs_gda_shrink": (_i, [C.POINTER(GdaParams), C.POINTER(GdaBuffers), _p]),
    "clipfs_gda_bias": (_i, [C.POINTER(GdaParams), C.POINTER(GdaBuffers), _p]),
    "clipfs_gda_search": (_i, [_p, _p, C.c_int, _p, _p, _p, C.c_int, C.c_int, C.c_int, _p]),
    "clipfs_gda_fit": (_i, [C.POINTER(GdaParams), C.POINTER(GdaBuffers), _p]),
    "clipfs_krr_plan": (_i, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(KrrPlan)]),
    "clipfs_krr_system": (_i, [_p, _p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, _p]),
    "clipfs_krr_targets": (_i, [_p, _p, _p, C.c_int, _p, C.c_int, C.c_int, C.c_int, C.c_float, _p]),
    "clipfs_krr_apply": (_i, [_p, _p, _p, C.c_int, _p, C.c_int, _p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _p]),
    "clipfs_krr_fit": (_i, [C.POINTER(KrrParams), C.POINTER(KrrBuffers), _p]),
    "clipfs_ot_plan": (_i, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(OtPlan)]),
    "clipfs_ot_logits": (_i, [_p, _p, _p, _p, _p, C.c_int, _p, _p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                              C.c_int, C.c_float, _p]),
    "clipfs_ot_bwd": (_i, [_p, _p, _p, _p, _p, C.c_int, _p, _p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                           C.c_float, C.c_int, _p]),
    "clipfs_augmix_plan": (_i, [_i, _i, _i, C.POINTER(AugmixPlan)]),
    "clipfs_augmix_batch": (_i, [_p, _sz, _p, _p, _i, _p, _p, _i, _i, _i, C.POINTER(AugmixRecipe), _p, _p, _p, _p, _p, _p]),
}

# word indices of the loss-scaling record (CLIPFS_SCALER_* of include/clipfs.h)
SCALER_SCALE, SCALER_INV_SCALE, SCALER_FOUND, SCALER_TRACKER, SCALER_STEP, SCALER_SKIPPED = 0, 1, 2, 3, 4, 5
SCALER_INV_SQRT_BC2, SCALER_STEP_SIZE, SCALER_SKIP, SCALER_WORDS = 6, 7, 8, 16
# word indices of the clip record (CLIPFS_CLIP_* of include/clipfs.h)
CLIP_NORM, CLIP_COEF, CLIP_MULT, CLIP_WORDS = 0, 1, 2, 8


def new_gemm_args() -> GemmArgs:
    g = GemmArgs()
    g.struct_size = C.sizeof(GemmArgs)
    return g


def gemm_f16_plan(g: GemmArgs, cus: int = 0):
    """[(kernel name, m_begin, m_end, side)] clipfs_gemm_nt would launch for the f16 x f16 product `g` (host-only)."""
    plan = F16Plan()
    check(load().clipfs_gemm_f16_plan(C.byref(g), cus, C.byref(plan)), "gemm_f16_plan")
    return [(F16_KERNELS[l.kernel], l.m_begin, l.m_end, bool(l.side)) for l in plan.launch[:plan.n]]


def gemm_plan(g: GemmArgs):
    """The plan clipfs_gemm_nt executes for the exact fp32 / 16-bit-plane product `g` (host-only), as a dict of the fields of
    struct clipfs_gemm_plan with the kernel by name.  A refusal raises ClipfsError with its message."""
    plan = GemmPlan()
    check(load().clipfs_gemm_plan(C.byref(g), C.byref(plan)), "gemm_plan")
    return dict(kernel=GEMM_KERNELS[plan.kernel], **{k: getattr(plan, k) for k, _ in GemmPlan._fields_[1:]})


def attention_plan(direction: str, batch: int, seq: int, heads: int, causal: bool, stats: bool = True, aligned: bool = True):
    """The plan clipfs_attention_fwd / _bwd and their packed forms execute for these arguments (host-only), as a dict:
    family, the family's own fields (nt | parts, tiles, ctok | lmax) and launches = ((grid_x, grid_y, block, lds_bytes), ...).
    A refusal raises ClipfsError with its message."""
    plan = AttentionPlan()
    flags = (ATTN_STATS if stats else 0) | (ATTN_ALIGNED if aligned else 0)
    check(load().clipfs_attention_plan(ATTN_DIRECTIONS.index(direction), batch, seq, heads, int(causal), flags, C.byref(plan)),
          "attention_plan")
    return _attention_plan_dict(plan)


def _attention_plan_dict(plan: AttentionPlan):
    own = {"mfma16": ("nt",), "mfma16_packed": ("nt",), "mfma16_pinned": ("nt",), "mfma_long": ("parts", "tiles", "ctok"),
           "recompute": ("lmax",), "f16_long": ("parts", "tiles", "ctok")}.get(ATTN_FAMILIES[plan.family], ())
    return dict(family=ATTN_FAMILIES[plan.family], **{k: getattr(plan, k) for k in own},
                launches=tuple((l.grid_x, l.grid_y, l.block, l.lds_bytes) for l in plan.launch[:plan.launches]))


def attention_f16_plan(direction: str, batch: int, seq: int, heads: int, causal: bool, stats: bool = True, aligned: bool = True):
    """The plan clipfs_attention_f16_fwd / _bwd / _bwd_packed execute for these arguments (host-only), as the dict of
    attention_plan: family "f16_short" or "f16_long" (with parts, tiles, ctok) and the launches.  A refusal raises
    ClipfsError with its message."""
    plan = AttentionPlan()
    flags = (ATTN_STATS if stats else 0) | (ATTN_ALIGNED if aligned else 0)
    check(load().clipfs_attention_f16_plan(ATTN_F16_DIRECTIONS.index(direction), batch, seq, heads, int(causal), flags,
                                           C.byref(plan)), "attention_f16_plan")
    return _attention_plan_dict(plan)


def lora_plan(op: str, rows: int, width: int, segw: int, r: int, nseg: int, x_act: bool = False, keep_bits: bool = False,
              frozen: bool = False, dx: bool = True):
    """The plan clipfs_lora_down / _bwd / _bwd_xact / _bwd_f16dy execute for these arguments (host-only), as a dict of the
    fields of struct clipfs_lora_plan with launches = ((grid_x, grid_y, block), ...).  A refusal raises ClipfsError with
    its message."""
    plan = LoraPlan()
    flags = (LORA_X_ACT if x_act else 0) | (LORA_KEEP_BITS if keep_bits else 0) | (LORA_FROZEN if frozen else 0) | (LORA_DX if dx else 0)
    check(load().clipfs_lora_plan(LORA_OPS.index(op), rows, width, segw, r, nseg, flags, C.byref(plan)), "lora_plan")
    d = {k: getattr(plan, k) for k, _ in LoraPlan._fields_[1:-2]}
    return dict(family=LORA_FAMILIES[plan.family], **d, launches=tuple((l.grid_x, l.grid_y, l.block) for l in plan.launch[:plan.launches]))


def cache_plan(op: str, B: int, NK: int, C_: int, d: int, nA: int = 1, nB: int = 1):
    """The plan clipfs_cache_logits / _bwd / _search execute for these shapes (host-only), as a dict of the fields of struct
    clipfs_cache_plan with grid = (x, y, z).  A refusal raises ClipfsError with its message."""
    plan = CachePlan()
    check(load().clipfs_cache_plan(CACHE_OPS.index(op), B, NK, C_, d, nA, nB, C.byref(plan)), "cache_plan")
    return dict(grid=(plan.grid_x, plan.grid_y, plan.grid_z), **{k: getattr(plan, k) for k, _ in CachePlan._fields_[3:]})


def contrastive_plan(op: str, R: int, N: int, d: int):
    """The plan clipfs_contrastive_objective executes for these shapes (host-only), as a dict of the fields of struct
    clipfs_contrastive_plan with grid = (x, y, z).  A refusal raises ClipfsError with its message."""
    plan = ContrastivePlan()
    check(load().clipfs_contrastive_plan(CONTRASTIVE_OPS.index(op), R, N, d, C.byref(plan)), "contrastive_plan")
    return dict(grid=(plan.grid_x, plan.grid_y, plan.grid_z), **{k: getattr(plan, k) for k, _ in ContrastivePlan._fields_[3:]})


def sigmoid_plan(op: str, R: int, N: int, d: int):
    """The plan clipfs_sigmoid_objective executes for these shapes (host-only), as a dict of the fields of struct
    clipfs_sigmoid_plan with grid = (x, y, z).  A refusal raises ClipfsError with its message."""
    plan = SigmoidPlan()
    check(load().clipfs_sigmoid_plan(SIGMOID_OPS.index(op), R, N, d, C.byref(plan)), "sigmoid_plan")
    return dict(grid=(plan.grid_x, plan.grid_y, plan.grid_z), **{k: getattr(plan, k) for k, _ in SigmoidPlan._fields_[3:]})


def clip_pairs_plan(op: str, R: int, N: int, d: int, both: bool = True):
    """The plan clipfs_clip_pairs_objective executes for these shapes (host-only; ``both``: weight_k != 0), as a dict of
    the fields of struct clipfs_clip_pairs_plan with grid = (x, y, z).  A refusal raises ClipfsError with its message."""
    plan = ClipPairsPlan()
    check(load().clipfs_clip_pairs_plan(CLIP_PAIRS_OPS.index(op), R, N, d, int(both), C.byref(plan)), "clip_pairs_plan")
    return dict(grid=(plan.grid_x, plan.grid_y, plan.grid_z), **{k: getattr(plan, k) for k, _ in ClipPairsPlan._fields_[3:]})


def new_tda_params(**fields) -> TdaParams:
    p = TdaParams()
    p.struct_size = C.sizeof(TdaParams)
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def tda_plan(params: TdaParams, B: int, update: bool = True):
    """The plan clipfs_tda_adapt executes (host-only), as a dict: launches (a count that does not depend on B or C), launch
    = {name: (grid_x, grid_y, block, lds_bytes)} of the launches present, lds_bytes, class_chunk and the state / record
    sizes of struct clipfs_tda_plan.  A refusal raises ClipfsError with its message."""
    plan = TdaPlan()
    check(load().clipfs_tda_plan(C.byref(params), B, int(update), C.byref(plan)), "tda_plan")
    d = {k: getattr(plan, k) for k, _ in TdaPlan._fields_ if k != "launch"}
    d["launch"] = {TDA_LAUNCHES[i]: (l.grid_x, l.grid_y, l.block, l.lds_bytes) for i, l in enumerate(plan.launch) if l.grid_x}
    return d


def new_transduct_params(**fields) -> TransductParams:
    p = TransductParams()
    p.struct_size = C.sizeof(TransductParams)
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def new_transduct_buffers(**members) -> TransductBuffers:
    """struct clipfs_transduct_buffers with the named members set (addresses as integers); the rest stay NULL."""
    b = TransductBuffers()
    b.struct_size = C.sizeof(TransductBuffers)
    for k, v in members.items():
        setattr(b, k, v)
    return b


def transduct_plan(params: TransductParams):
    """The plan the transductive entry points execute (host-only), as a dict of the fields of struct clipfs_transduct_plan with
    launch = {name: (grid_x, grid_y, grid_z, block, lds_bytes)} of the launches present.  A refusal raises ClipfsError."""
    plan = TransductPlan()
    check(load().clipfs_transduct_plan(C.byref(params), C.byref(plan)), "transduct_plan")
    d = {k: getattr(plan, k) for k, _ in TransductPlan._fields_ if k != "launch"}
    d["launch"] = {TRANSDUCT_LAUNCHES[i]: (l.grid_x, l.grid_y, l.grid_z, l.block, l.lds_bytes)
                   for i, l in enumerate(plan.launch) if l.grid_x}
    return d


def spd_plan(n: int, nrhs: int = 1):
    """The plan clipfs_spd_factor / clipfs_spd_solve execute for an n x n system with nrhs right-hand sides (host-only), as a
    dict of the fields of struct clipfs_spd_plan.  A refusal raises ClipfsError with its message."""
    plan = SpdPlan()
    check(load().clipfs_spd_plan(n, nrhs, C.byref(plan)), "spd_plan")
    return {k: getattr(plan, k) for k, _ in SpdPlan._fields_}


def new_gda_params(**fields) -> GdaParams:
    p = GdaParams()
    p.struct_size = C.sizeof(GdaParams)
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def new_gda_buffers(**members) -> GdaBuffers:
    """struct clipfs_gda_buffers with the named members set (addresses as integers); the rest stay NULL."""
    b = GdaBuffers()
    b.struct_size = C.sizeof(GdaBuffers)
    for k, v in members.items():
        setattr(b, k, v)
    return b


def gda_plan(params: GdaParams):
    """The plan the GDA entry points execute (host-only), as a dict of the fields of struct clipfs_gda_plan.  A refusal raises
    ClipfsError with its message."""
    plan = GdaPlan()
    check(load().clipfs_gda_plan(C.byref(params), C.byref(plan)), "gda_plan")
    return {k: getattr(plan, k) for k, _ in GdaPlan._fields_}


def spd_panels_plan(n: int, nrhs: int = 1, panel: int = 256):
    """The plan clipfs_spd_factor_panels / clipfs_spd_solve_panels execute (host-only), as a dict of the fields of struct
    clipfs_spd_panels_plan.  A refusal raises ClipfsError with its message."""
    plan = SpdPanelsPlan()
    check(load().clipfs_spd_panels_plan(n, nrhs, panel, C.byref(plan)), "spd_panels_plan")
    return {k: getattr(plan, k) for k, _ in SpdPanelsPlan._fields_}


def new_krr_params(**fields) -> KrrParams:
    p = KrrParams()
    p.struct_size = C.sizeof(KrrParams)
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def new_krr_buffers(**members) -> KrrBuffers:
    """struct clipfs_krr_buffers with the named members set (addresses as integers); the rest stay NULL / 0."""
    b = KrrBuffers()
    b.struct_size = C.sizeof(KrrBuffers)
    for k, v in members.items():
        setattr(b, k, v)
    return b


def krr_plan(n: int, C_: int, d: int, B: int = 1, panel: int = 256):
    """The plan clipfs_krr_fit / clipfs_krr_apply execute (host-only), as a dict of the fields of struct clipfs_krr_plan.  A
    refusal raises ClipfsError with its message."""
    plan = KrrPlan()
    check(load().clipfs_krr_plan(n, C_, d, B, panel, C.byref(plan)), "krr_plan")
    return {k: getattr(plan, k) for k, _ in KrrPlan._fields_}


def ot_plan(B: int, M: int, C_: int, N: int, d: int):
    """The plan clipfs_ot_logits / clipfs_ot_bwd execute for B images of M rows against C_ classes of N prompts (host-only), as
    a dict of the fields of struct clipfs_ot_plan.  A refusal raises ClipfsError with its message."""
    plan = OtPlan()
    check(load().clipfs_ot_plan(B, M, C_, N, d, C.byref(plan)), "ot_plan")
    return {k: getattr(plan, k) for k, _ in OtPlan._fields_}


def augmix_plan(n: int, S: int, width: int):
    """The plan clipfs_augmix_batch executes for n views of side S with ``width`` chains (host-only), as a dict of the fields
    of struct clipfs_augmix_plan with launch = {name: (grid_x, grid_y, block, lds_bytes)}.  A refusal raises ClipfsError
    with its message."""
    plan = AugmixPlan()
    check(load().clipfs_augmix_plan(n, S, width, C.byref(plan)), "augmix_plan")
    d = {k: getattr(plan, k) for k, _ in AugmixPlan._fields_ if k != "launch"}
    d["launch"] = {AUGMIX_LAUNCHES[i]: (l.grid_x, l.grid_y, l.block, l.lds_bytes) for i, l in enumerate(plan.launch)}
    return d


def new_tower() -> Tower:
    t = Tower()
    t.struct_size = C.sizeof(Tower)
    t.block_size = C.sizeof(Block)
    return t


_lib = None


def load() -> C.CDLL:
    """dlopen the in-tree library (after torch, so the HIP runtime PyTorch already loaded is the one
    the library binds to: both carry SONAME libamdhip64.so.7)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise ClipfsError(
            f"{LIB_PATH} not found: the HIP engine is not built.  Run "
            "`python jittor-clip-fewshot_amd/build.py` (needs hipcc).  There is no CPU fallback.")
    try:
        import torch  # noqa: F401  (loads torch's libamdhip64 first)
    except Exception:  # pragma: no cover - symbol-export checks may run without torch
        pass
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL if hasattr(C, "RTLD_GLOBAL") else 0)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here == header/library mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    if lib.clipfs_abi_version() != ABI_VERSION:
        raise ClipfsError(f"libclipfs_hip.so ABI version {lib.clipfs_abi_version()} != {ABI_VERSION} of this binding: "
                          "rebuild with `python jittor-clip-fewshot_amd/build.py --force`")
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().clipfs_last_error().decode("utf-8", "replace")
        raise ClipfsError(f"{what or 'clipfs call'} failed (rc={rc}): {msg}")
